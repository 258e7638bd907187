"""HipThresholdHitStream on ragged, mixed-layout, shuffled and sparse runs (tests/stream_hits_util.py) against the oracle
over the whole run and against HipThresholdHitPlugin on the same Context: through compute() serial and parallel, through
run_chunks on rings of every size, chunk by chunk through compute_chunk with the profile naming each chunk's route.

The plugin is constructed WITHOUT max_len throughout: the padded width of every chunk has to be the run's longest record
(hit_finder.py:364,370), or the rows that end near a short record's end differ from hit_threshold's in position, height,
integral, rise / fall time and timestamp.  tests/test_stream_hits_cpu.py counts those rows in the inputs."""

import functools

import numpy as np
import pytest

from tests import golden_util as G
from tests import stream_hits_util as S
from tests.test_hip_layout_routes import ROUTES, STAGE, _names
from waveformanalysis_amd.device import DevicePool, device_count
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipThresholdHitPlugin
from waveformanalysis_amd.streaming import HipThresholdHitStream

pytestmark = pytest.mark.gpu
FLOAT_RTOL = 1e-6          # the bar of tests/test_hip_parity.py and tests/test_hip_layout_routes.py for a hit row's floats
CASES = [(name, f) for name in S.RUN_NAMES for f in (False, True)]
TABLES: dict = {}          # (run, use_filtered, chunk_size) -> the first table a driver gave for that chunk list


@pytest.fixture(scope="module")
def dp():
    pool = DevicePool([0])
    yield pool
    pool.close()


def _ctx(run, config=None):
    return SimpleContext({"wave_source": "records", **(config or {})}, {"records": run.records, "wave_pool": run.pool})


@functools.cache
def _static_rows(name, use_filtered):
    """hit_threshold of the whole run: the static plugin on the records route, the fused SG(11, 2) for use_filtered."""
    run = S.run(name)
    cfg = {"threshold": S.THRESHOLD, "left_extension": S.LE, "right_extension": S.RE}
    if use_filtered:
        cfg.update(use_filtered=True, fuse_filter=True)
    ctx = SimpleContext({"wave_source": "records", "hit_threshold": cfg}, {"records": run.records, "wave_pool": run.pool},
                        plugins=[HipThresholdHitPlugin()])
    rows = ctx.get_data("run", "hit_threshold")
    rows.setflags(write=False)
    return rows


def _check(run, use_filtered, c, chunks, outs, what):
    """Bookkeeping, rows against the run-wide oracle and against the static plugin, bytes against the other drivers."""
    want = run.want(use_filtered)
    got = S.check_bookkeeping(run, chunks, outs, want, what)
    G.assert_struct_equal(got, want, float_rtol=FLOAT_RTOL, what=f"{what} vs oracle")
    G.assert_struct_equal(got, _static_rows(run.name, use_filtered), float_rtol=FLOAT_RTOL, what=f"{what} vs hit_threshold")
    for k, (ch, o) in enumerate(zip(chunks, outs)):     # every chunk complete by itself
        assert len(o.data) == int(np.isin(want["record_id"], ch.data["record_id"]).sum()), (what, k)
    first = TABLES.setdefault((run.name, use_filtered, c), got)
    assert got.tobytes() == first.tobytes(), f"{what}: rows differ from another driver's over the same chunks"
    return got


@pytest.mark.parametrize("name,use_filtered", CASES)
def test_compute_serial_and_parallel(name, use_filtered, dp):
    run = S.run(name)
    ctx = _ctx(run)
    plugin = HipThresholdHitStream(use_filtered=use_filtered, device_pool=dp)
    for c in run.chunk_sizes:
        chunks = run.chunks(c)
        for cfg in ({"chunk_size": c, "parallel": False}, {"chunk_size": c, "max_workers": 2},
                    {"chunk_size": c, "max_workers": 3}):
            outs = list(plugin.compute(ctx, "run", streaming_config=cfg))
            got = _check(run, use_filtered, c, chunks, outs, f"{name} filtered={use_filtered} compute {cfg}")
            assert [o.metadata["segment_id"] for o in outs] == [ch.metadata["segment_id"] for ch in chunks]
            if name == "mixed":
                assert {o.metadata["segment_id"] for o in outs} == {0, 1, 2, 3}
        print(f"{name} filtered={use_filtered} chunk_size={c}: {len(got)} rows, {int(run.in_padding(got).sum())} of them "
              f"in the padding, {len(chunks)} chunks")


@pytest.mark.parametrize("name,use_filtered", CASES)
def test_run_chunks_on_rings_of_every_size(name, use_filtered, dp):
    run = S.run(name)
    ctx = _ctx(run)
    plugin = HipThresholdHitStream(use_filtered=use_filtered, device_pool=dp)
    for c in run.chunk_sizes:
        chunks = run.chunks(c)
        for w in (1, 2, 8):
            timeline = []
            outs = plugin.run_chunks(chunks, ctx, "run", max_workers=w, timeline=timeline)
            _check(run, use_filtered, c, chunks, outs, f"{name} filtered={use_filtered} run_chunks c={c} workers={w}")
            assert [t[0] for t in timeline] == (list(range(len(chunks))) if w > 1 else [])


@pytest.mark.parametrize("name,use_filtered", CASES)
def test_run_chunks_on_every_visible_device(name, use_filtered):
    n = device_count()
    if n < 2:
        pytest.skip("1 device visible: the every-device ring needs two or more")
    run = S.run(name)
    pool = DevicePool(list(range(n)))
    try:
        plugin = HipThresholdHitStream(use_filtered=use_filtered, device_pool=pool)
        c = run.chunk_sizes[0]
        chunks = run.chunks(c)
        for w in (2, 8):
            outs = plugin.run_chunks(chunks, _ctx(run), "run", max_workers=w)
            _check(run, use_filtered, c, chunks, outs, f"{name} filtered={use_filtered} {n} devices workers={w}")
    finally:
        pool.close()


def test_constructor_width_below_the_run_is_refused(dp):
    run = S.run("ragged")
    plugin = HipThresholdHitStream(max_len=199, device_pool=dp)
    with pytest.raises(ValueError, match="below the longest record of the run"):
        plugin.run_chunks(run.chunks(100), _ctx(run), "run", max_workers=2)
    # a wider matrix than the run's is what the constructor may ask for: the rows of the oracle at that width
    from tests.hit_rows_util import oracle_rows

    outs = HipThresholdHitStream(max_len=203, device_pool=dp).run_chunks(run.chunks(100), _ctx(run), "run", max_workers=2)
    want = oracle_rows(run.records, run.pool, np.full(len(run.records), S.THRESHOLD), S.LE, S.RE, max_len=203)
    G.assert_struct_equal(np.concatenate([o.data for o in outs]), want, float_rtol=FLOAT_RTOL, what="max_len=203")


# ---- routes -----------------------------------------------------------------------------------------------------------
def test_queued_passes_take_every_layout_route():
    """compute_chunk chunk by chunk on the one session of a pool, the profile on: the chunks of one mixed run take the
    streaming kernel in place (L64), on the padded shadow (L88) and the per-record mask kernel (ragged, L24), the routes
    tests/test_hip_layout_routes.ROUTES names for these layouts."""
    run = S.run("mixed")
    ctx = _ctx(run)
    chunks = run.chunks(100)
    one = DevicePool([0], max_sessions=1)
    try:
        plugin = HipThresholdHitStream(use_filtered=True, device_pool=one)
        seen, outs = [], []
        for ch in chunks:
            with one.borrow() as sess:
                sess.profile(True)
            outs.append(plugin.compute_chunk(ch, ctx, "run"))
            with one.borrow() as sess:
                report = set(sess.profile_report())
            layout = S.MIXED_SEGMENTS[ch.metadata["segment_id"]][0]
            assert _names(report) & STAGE == ROUTES[layout][0][""], (layout, len(ch.data), report)
            seen.append(frozenset(_names(report) & STAGE))
        assert one.live_sessions == 1
        _check(run, True, 100, chunks, outs, "mixed compute_chunk with the profile on")
        assert frozenset({"k_sg_runs32"}) in seen and frozenset({"k_pad_rows", "k_sg_runs32"}) in seen
        assert frozenset({"k_sg_mask"}) in seen       # neither fast route: no streaming kernel, no span kernel
        assert len(set(seen)) == 3
        # the raw source has one route for every layout
        plugin = HipThresholdHitStream(use_filtered=False, device_pool=one)
        with one.borrow() as sess:
            sess.profile(True)
        outs = [plugin.compute_chunk(ch, ctx, "run") for ch in chunks]
        with one.borrow() as sess:
            report = set(sess.profile_report())
        assert any(k.startswith("k_hits<raw>") for k in report) and not _names(report) & STAGE - {"k_hits"}, report
        _check(run, False, 100, chunks, outs, "mixed raw compute_chunk with the profile on")
    finally:
        one.close()


# ---- ring -------------------------------------------------------------------------------------------------------------
def test_ring_is_a_double_buffer_and_keeps_its_sessions():
    run = S.run("mixed")
    ctx = _ctx(run)
    chunks = run.chunks(100)
    pool = DevicePool([0])
    try:
        plugin = HipThresholdHitStream(use_filtered=True, device_pool=pool)
        for _call in range(3):
            timeline = []
            outs = plugin.run_chunks(chunks, ctx, "run", max_workers=3, timeline=timeline)
            assert [t[0] for t in timeline] == list(range(len(chunks)))
            # chunk k + 1 is staged and queued before anybody waits for chunk k
            for (k, _b, queued, collected), (_k1, begin1, queued1, _c1) in zip(timeline, timeline[1:]):
                assert queued <= begin1 <= queued1 <= collected, (k, timeline)
            _check(run, True, 100, chunks, outs, "mixed ring")
            assert pool.live_sessions == 2      # two sessions for one device, the same ones in every call
    finally:
        pool.close()


# ---- sparse -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_filtered", [False, True])
def test_sparse_chunks_and_a_chunk_of_no_records(use_filtered, dp):
    run = S.run("sparse")
    ctx = _ctx(run)
    want = run.want(use_filtered)
    chunks, k_empty = S.sparse_chunks_with_empty()
    plugin = HipThresholdHitStream(use_filtered=use_filtered, device_pool=dp)
    first = None
    for w in (1, 2, 3):
        outs = plugin.run_chunks(chunks, ctx, "run", max_workers=w)
        got = S.check_bookkeeping(run, chunks, outs, want, f"sparse workers={w}")
        G.assert_struct_equal(got, want, float_rtol=FLOAT_RTOL, what=f"sparse filtered={use_filtered} workers={w}")
        assert len(outs[k_empty].data) == 0
        assert (outs[k_empty].start, outs[k_empty].end) == (chunks[k_empty].start, chunks[k_empty].end)
        # a chunk without a hit, then a complete one: the rows of every chunk are the oracle's rows of its records
        pattern = list(S.SPARSE_PATTERN)
        pattern.insert(k_empty, False)
        for k, (ch, o) in enumerate(zip(chunks, outs)):
            sel = np.isin(want["record_id"], ch.data["record_id"])
            assert (len(o.data) > 0) == pattern[k] and len(o.data) == int(sel.sum()), (w, k)
            G.assert_struct_equal(o.data, want[sel], float_rtol=FLOAT_RTOL, what=f"sparse workers={w} chunk {k}")
        first = got if first is None else first
        assert got.tobytes() == first.tobytes()
    # a threshold no sample reaches (from the Context): every chunk is a miss, every result is there and empty
    miss = _ctx(run, {"threshold": 1e9})
    outs = list(plugin.compute(miss, "run", streaming_config={"chunk_size": S.SPARSE_BLOCK, "max_workers": 2}))
    assert len(outs) == len(S.SPARSE_PATTERN) and all(len(o.data) == 0 for o in outs)
    outs = plugin.run_chunks(chunks, ctx, "run", max_workers=2)     # and the same sessions give the full rows again
    assert np.concatenate([o.data for o in outs]).tobytes() == first.tobytes()
