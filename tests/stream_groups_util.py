"""Inputs and expectations for the streaming hit pipeline under per-channel settings (HipThresholdHitStream with
channel_config and filter_source="wave_pool_filtered"): tests/test_stream_groups_cpu.py, tests/test_hip_stream_groups.py.

Configuration: FILTER_CC / HIT_CC of tests/fused_groups_util.py (channel 0 SG(11, 2), 1 SG(7, 3), 2 SG(21, 4), 3
Butterworth; thresholds 10 / 2 / 10 / 3), and an SG-only variant in which channel 3 takes SG(9, 2): every group of it is a
fused Savitzky-Golay pass, so every group can take a speculative route.

Runs: the three runs of the fixture tests/golden/c5_fused_groups.npz (the reference's rows), the four runs of
tests/stream_hits_util.py (records on channels k % 4 of board 0) and `missing`: the ragged run with its channels
rewritten per block of 50 records -- all four channels, only channel 0, only channels 1 and 3, and so on -- so that chunks
of 50 records lack groups.  The expectation is the oracle over the whole run (`want`), never over a chunk.

`GroupOracleSession` is a device double that answers the session calls of the grouped pass with the oracle."""

from __future__ import annotations

import functools

import numpy as np

from oracle import wfa_oracle as O
from tests import fused_groups_util as F
from tests import hit_rows_util as H
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib
from waveformanalysis_amd.plugin_api import SimpleContext

FILTER_CC, HIT_CC = F.FILTER_CC, F.HIT_CC
SG_ONLY_CC = dict(FILTER_CC, **{"0:3": {"sg_window_size": 9, "sg_poly_order": 2}})
KEYS = {"full": list(F.KEYS), "sg_only": list(F.KEYS[:3]) + [("SG", 9, 2)]}
CONFIGS = {"full": FILTER_CC, "sg_only": SG_ONLY_CC}
THRESHOLDS = np.asarray(F.THRESHOLDS)
LE, RE = S.LE, S.RE
RUN_NAMES = S.RUN_NAMES + ("missing",)
MISSING_BLOCK = 50
MISSING_PATTERN = ((0, 1, 2, 3), (0,), (1, 3))     # the channels of consecutive blocks of MISSING_BLOCK records


@functools.cache
def missing() -> S.Run:
    base = S.ragged()
    rec = base.records.copy()
    k = np.arange(len(rec))
    for b in range(0, len(rec), MISSING_BLOCK):
        chans = MISSING_PATTERN[(b // MISSING_BLOCK) % len(MISSING_PATTERN)]
        rec["channel"][b : b + MISSING_BLOCK] = np.asarray(chans)[k[b : b + MISSING_BLOCK] % len(chans)]
    rec.setflags(write=False)
    return S.Run("missing", rec, base.pool, (MISSING_BLOCK,))


def run(name: str) -> S.Run:
    return missing() if name == "missing" else S.run(name)


@functools.cache
def exceeding_run() -> tuple[np.ndarray, np.ndarray]:
    """(records, pool) of a run whose groups outgrow the smallest speculative row bound: 12 000 uniform records of 64
    samples with two hits each over four channels, about 6000 rows per channel, against the 4096 + 4096 / 8 rows a
    launch is sized for behind a pass that found nothing.  A grouped call over it on a context whose previous calls
    found nothing returns with the pass pending, and wfa_hits_wait redoes it the exact way."""
    n, L = 12_000, 64
    rng = np.random.default_rng(31)
    pool = np.concatenate([S._wave(L, 4, rng) for _ in range(n)])       # two hits per record
    rec = S._records(np.full(n, L), np.arange(n, dtype=np.int64) * L, 10**12 + np.arange(n, dtype=np.int64) * 300_000)
    rec.setflags(write=False)
    pool.setflags(write=False)
    return rec, pool


def filter_kwargs(key: tuple) -> dict:
    """A filter key of filter_engine.resolve_filter_key as the oracle's keyword arguments."""
    if key[0] == "BW":
        return {"filter_type": "BW", "bw_sos": O.design_bw(*key[1:])}
    return {"filter_type": "SG", "sg_window_size": key[1], "sg_poly_order": key[2]}


def oracle_filtered(records: np.ndarray, pool: np.ndarray, keys: list) -> np.ndarray:
    """O.filter_wave_pool with the filter of every record's channel (keys[channel])."""
    kw = [filter_kwargs(k) for k in keys]
    chan = records["channel"]
    return O.filter_wave_pool(records, pool, per_record_cfg=lambda i: kw[int(chan[i])])


@functools.cache
def want(name: str, config: str = "full") -> np.ndarray:
    """The run-wide oracle under the configuration.  Asserted here, so that nothing passes vacuously: at least 20 rows
    per group, a table that differs from the uniform filter's, and for `missing` a chunk with one group and one with two."""
    r = run(name)
    rows = O.threshold_hits(r.records, oracle_filtered(r.records, r.pool, KEYS[config]),
                            thresholds=THRESHOLDS[r.records["channel"]], left_extension=LE, right_extension=RE)
    rows.setflags(write=False)
    per_channel = np.bincount(rows["channel"], minlength=4)
    assert np.all(per_channel >= 20), (name, config, per_channel)
    uniform = r.want(True)
    assert len(uniform) != len(rows) or uniform.tobytes() != rows.tobytes(), (name, config)
    if name == "missing":
        groups = [len(np.unique(c.data["channel"])) for c in r.chunks(MISSING_BLOCK)]
        assert 1 in groups and 2 in groups and 4 in groups, groups
    else:
        for c in r.chunk_sizes:
            assert all(len(np.unique(ch.data["channel"])) == 4 for ch in r.chunks(c)), (name, c)
    return rows


def stream_config(config: str = "full") -> dict:
    return {"threshold": S.THRESHOLD, "left_extension": LE, "right_extension": RE, "use_filtered": True,
            "filter_source": "wave_pool_filtered", "channel_config": HIT_CC}


def context(records: np.ndarray, pool: np.ndarray, config: str = "full", extra: dict | None = None) -> SimpleContext:
    """A Context with the configuration on hit_threshold (fused), wave_pool_filtered and hit_threshold_stream."""
    from waveformanalysis_amd.plugins import HipThresholdHitPlugin, HipWavePoolFilteredPlugin

    hit = {"threshold": S.THRESHOLD, "left_extension": LE, "right_extension": RE, "use_filtered": True, "fuse_filter": True,
           "channel_config": HIT_CC}
    return SimpleContext({"wave_source": "records", "hit_threshold": hit,
                          "wave_pool_filtered": {"channel_config": CONFIGS[config]},
                          "hit_threshold_stream": stream_config(config), **(extra or {})},
                         {"records": records, "wave_pool": pool},
                         plugins=[HipWavePoolFilteredPlugin(), HipThresholdHitPlugin()])


# ---- a device double that computes -----------------------------------------------------------------------------------
class GroupOracleSession(S.OracleSession):
    """OracleSession with the session calls of the grouped pass: plan slots, the Butterworth filter of one group, the
    queued grouped pass (the oracle's rows per group, merged by record index) and hits_pending.  `calls` (shared by the
    sessions of one factory) receives the name of every device call in order."""

    def __init__(self, device_id: int = 0, log: list | None = None, uploads: list | None = None, calls: list | None = None):
        super().__init__(device_id, log, uploads)
        self.calls = [] if calls is None else calls
        self._slots: dict = {}
        self._twin = None
        self._queued = False

    def upload_pool(self, pool):
        self.calls.append("upload_pool")
        super().upload_pool(pool)
        self._twin = None

    def upload_records(self, rec, thr):
        self.calls.append("upload_records" if isinstance(thr, float) else "upload_records[]")   # a float, or a column
        thr = np.asarray(thr, dtype=np.float64)
        S.Session.upload_records(self, rec, thr)
        self._rec, self._thr = rec.copy(), thr
        self.n_records = len(rec)

    def set_sg_plan(self, w, p):
        self.calls.append("set_sg_plan")
        super().set_sg_plan(w, p)

    def store_sg_plan(self, slot, w, p):
        self.calls.append("store_sg_plan")
        assert 0 <= slot < _lib.MAX_HIT_GROUPS
        self._slots[int(slot)] = (int(w), int(p))

    def sosfiltfilt_group(self, sos, zi, padlen, group_of_record, group):
        self.calls.append("sosfiltfilt_group")
        assert self._rec is not None and len(group_of_record) == len(self._rec)
        if self._twin is None:
            self._twin = np.zeros(len(self._pool), dtype=np.float32)
        mine = np.asarray(group_of_record) == group
        part = O.filter_wave_pool(self._rec[mine], self._pool, "BW", bw_sos=np.asarray(sos))
        for o, n in zip(self._rec["wave_offset"][mine], self._rec["event_length"][mine]):
            self._twin[o : o + n] = part[o : o + n]

    def _thresholds(self):
        return np.broadcast_to(self._thr, (len(self._rec),)).astype(np.float64)

    def hits_enqueue(self, source=_lib.SRC_SG_FUSED, baseline_window=(0, 0), left_extension=2, right_extension=2, max_len=0):
        self.calls.append("hits_enqueue")
        if np.ndim(self._thr) == 0:
            self._thr = float(self._thr)
            return super().hits_enqueue(source, baseline_window, left_extension, right_extension, max_len)
        rec, pool = self._rec, self._pool
        self.log.append({"device": self.device_id, "session": self, "max_len": int(max_len), "source": int(source),
                         "n_records": len(rec), "pool": pool, "records": rec})
        src = pool if source == _lib.SRC_RAW else O.filter_wave_pool(rec, pool, sg_window_size=self._sg[0],
                                                                     sg_poly_order=self._sg[1])
        self._rows = H.oracle_rows(rec, src, self._thresholds(), left_extension, right_extension, int(max_len))
        self._queued = True

    def hits_enqueue_groups(self, groups, group_of_record, left_extension=2, right_extension=2, max_len=0,
                            baseline_window=(0, 0)):
        self.calls.append("hits_enqueue_groups")
        assert tuple(baseline_window) == (0, 0), "the stream passes no baseline window"
        rec, pool = self._rec, self._pool
        gor = np.asarray(group_of_record)
        assert 1 <= len(groups) <= _lib.MAX_HIT_GROUPS and len(gor) == len(rec)
        assert gor.min() >= -1 and gor.max() < len(groups)
        longest = int(rec["event_length"].max())
        if 0 < max_len < longest:
            raise _lib.WfaError(_lib.WFA_E_INVALID, f"max_len ({max_len}) < longest uploaded record ({longest})")
        self.log.append({"device": self.device_id, "session": self, "max_len": int(max_len), "groups": list(groups),
                         "n_records": len(rec), "pool": pool, "records": rec, "group_of_record": gor.copy()})
        own = self._thresholds()
        parts = []
        for g, (source, slot) in enumerate(groups):
            if source == _lib.SRC_F32:
                assert self._twin is not None, "an F32 group without its filter call"
                src = self._twin
            else:
                w, p = self._slots[slot]
                src = O.filter_wave_pool(rec, pool, sg_window_size=w, sg_poly_order=p)
            parts.append(H.oracle_rows(rec, src, np.where(gor == g, own, np.inf), left_extension, right_extension, int(max_len)))
        self._rows = F.host_merge(rec, parts)
        self._queued = True

    def hits_pending(self):
        return self._queued

    def hits_wait(self):
        self._queued = False
        return super().hits_wait()


def oracle_pool(device_ids=(0,), **kw):
    """A DevicePool of GroupOracleSessions that share one log, one list of uploads and one list of call names."""
    from waveformanalysis_amd.device import DevicePool

    log, uploads, calls = [], [], []
    pool = DevicePool(device_ids=list(device_ids),
                      session_factory=lambda dev: GroupOracleSession(dev, log, uploads, calls), **kw)
    pool.log, pool.uploads, pool.calls = log, uploads, calls
    return pool
