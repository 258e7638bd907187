"""The merge stream's rule restated in numpy, and a device double that answers the merge stream calls with it.

`NumpyMergeStream` is the stream on top of the oracle's literal chain (oracle.wfa_oracle.hit_merge_clusters /
hit_merged_rows): carry ++ new rows, per channel the clusters no later hit can precede or join, carry in original row order.
It is written against the rule, not against the library: the CPU tests compare it, through `static_tables`, with the tables
the reference recorded, the GPU tests compare the library with it push by push.
"""

from __future__ import annotations

import math

import numpy as np

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests.event_stream_util import make_hits, row_horizons, windows_of
from tests.stream_hits_util import OracleSession
from waveformanalysis_amd.dtypes import HIT_MERGED_DTYPE, THRESHOLD_HIT_DTYPE

FIXTURES = ("merge_crafted", "merge_v1725")
CPU_CHUNK_SIZES = (1, 2, 3, 7, 64, "n", "n+1")


def chunk_size_of(spec, n: int) -> int:
    return {"n": n, "n+1": n + 1}.get(spec, spec)


def fixture(name: str) -> dict:
    """hits, configs (list of {merge_gap_ns, max_total_width_ns}) and clusters_k / merged_k / components_k."""
    return G.load_merge(name)


class NumpyMergeStream:
    """push(rows, horizon) -> (merged rows, hit_index, rows carried, open_start)."""

    def __init__(self, merge_gap_ns: float = 0.0, max_total_width_ns: float = 10000.0):   # hit_merged's defaults
        self.gap_ns, self.width_ns = float(merge_gap_ns), float(max_total_width_ns)
        self.carry = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)
        self.index = np.zeros(0, dtype=np.int64)
        self.next_hit = self.next_component = self.max_carry = 0

    def push(self, rows, horizon: float):
        new = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE) if rows is None else np.asarray(rows)
        table = np.concatenate([self.carry, new])
        index = np.concatenate([self.index, self.next_hit + np.arange(len(new), dtype=np.int64)])
        self.next_hit += len(new)
        a0, a1 = windows_of(table)
        gap_ps = self.gap_ns * 1e3
        closed, position, final = [], {}, {}
        for members in O.hit_merge_clusters(table, self.gap_ns, self.width_ns):   # channel-major, chain order
            key = (int(table["board"][members[0]]), int(table["channel"][members[0]]))
            if key not in final:                                                    # F of the channel
                final[key] = int(np.sum((table["board"] == key[0]) & (table["channel"] == key[1]) & (a0 < horizon)))
            b = position[key] = position.get(key, 0) + len(members)
            if b <= final[key] and (b < final[key] or self.gap_ns <= 0
                                    or np.float64(horizon) - np.float64(a1[members].max()) > gap_ps):
                closed.append(members)
        merged = O.hit_merged_rows(table, closed).astype(HIT_MERGED_DTYPE)
        merged["component_offset"] += self.next_component
        flat = np.array([i for members in closed for i in members], dtype=np.int64)
        self.next_component += len(flat)
        keep = np.ones(len(table), dtype=bool)
        keep[flat] = False
        self.carry, self.index = table[keep], index[keep]                           # original row order
        self.max_carry = max(self.max_carry, len(self.carry))
        open_start = float(a0[keep].min()) if keep.any() else math.inf
        return merged, index[flat], len(self.carry), open_start


def stream_all(push, hits: np.ndarray, chunk_size: int, horizons: list | None = None):
    """Everything `push(rows, horizon) -> (merged, hit_index, n_carry, open_start)` delivers for `hits` in chunks of
    chunk_size, plus the flush: (merged rows, hit_index), concatenated in delivery order."""
    horizons = row_horizons(hits, chunk_size) if horizons is None else horizons
    rows, members = [np.zeros(0, dtype=HIT_MERGED_DTYPE)], [np.zeros(0, dtype=np.int64)]
    for k, lo in enumerate(range(0, len(hits), chunk_size)):
        out = push(hits[lo : lo + chunk_size], horizons[k])
        rows.append(out[0])
        members.append(out[1])
    out = push(None, math.inf)
    assert out[2] == 0 and out[3] == math.inf
    rows.append(out[0])
    members.append(out[1])
    merged = np.concatenate(rows)
    assert np.array_equal(merged["component_offset"], np.cumsum(merged["component_count"]) - merged["component_count"])
    return merged, np.concatenate(members)


# ---- device doubles -----------------------------------------------------------------------------------------------------
class MergeOracleSession(OracleSession):
    """OracleSession that also answers the merge stream calls with NumpyMergeStream and records them in `calls`."""

    def __init__(self, device_id: int = 0, log=None, uploads=None, calls=None):
        super().__init__(device_id, log, uploads)
        self.calls = [] if calls is None else calls
        self._stream = None

    def merge_stream_begin(self, merge_gap_ns, max_total_width_ns):
        self.calls.append(("begin", float(merge_gap_ns), float(max_total_width_ns), self))
        self._stream = NumpyMergeStream(merge_gap_ns, max_total_width_ns)

    def merge_stream_push(self, rows, horizon):
        assert self._stream is not None, "push without begin"
        self.calls.append(("push", 0 if rows is None else len(rows), float(horizon), self))
        return self._stream.push(rows, horizon)

    def merge_stream_end(self):
        self.calls.append(("end", self))
        self._stream = None


def merge_pool(device_ids=(0,), **kw):
    from waveformanalysis_amd.device import DevicePool

    log, uploads, calls = [], [], []
    pool = DevicePool(device_ids=list(device_ids),
                      session_factory=lambda dev: MergeOracleSession(dev, log, uploads, calls), **kw)
    pool.log, pool.uploads, pool.calls = log, uploads, calls
    return pool


__all__ = ["NumpyMergeStream", "MergeOracleSession", "merge_pool", "stream_all", "fixture", "FIXTURES", "CPU_CHUNK_SIZES",
           "chunk_size_of", "make_hits", "row_horizons", "windows_of", "THRESHOLD_HIT_DTYPE"]
