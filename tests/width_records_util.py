"""The records route of waveform_width: fixture loading (tests/golden/c5_width_records.npz, made with the reference by
tests/golden/make_width_records_golden.py) and the oracle applied per record."""

from __future__ import annotations

import json
import os
import warnings

import numpy as np

from oracle import wfa_oracle as O
from tests import golden_util as G
from waveformanalysis_amd.dtypes import WAVEFORM_WIDTH_DTYPE

FIXTURE = os.path.join(G.GOLDEN, "c5_width_records.npz")
TABLES = ("raw", "filt", "crafted")
POOLS = {"u16": "wave_pool", "f32": "wave_pool_filtered"}
REQUIRED_LENGTHS = (0, 1, 7, 8, 13, 17, 49, 50, 51, 64, 65, 800, 1500)

_cache: dict = {}


def load() -> dict:
    """The fixture's arrays (shared, read-only) + `options`: the four option sets."""
    if not _cache:
        z = np.load(FIXTURE, allow_pickle=False)
        for k in z.files:
            _cache[k] = z[k]
            _cache[k].setflags(write=False)
        _cache["options"] = json.loads(bytes(_cache.pop("options_json")).decode())
    return _cache


def oracle_widths(hits: np.ndarray, records: np.ndarray, pool: np.ndarray, **options) -> np.ndarray:
    """O.waveform_width per record on a one-row dense array holding the record's slice; rows in hit order.  The hit's
    record_id is an index into `records`; ids outside the table have no row."""
    rid = np.asarray(hits["record_id"], dtype=np.int64)
    parts, order = [], []
    for r in np.unique(rid):
        if not 0 <= r < len(records):
            continue
        off, L = int(records["wave_offset"][r]), int(records["event_length"][r])
        row = np.zeros(1, dtype=[("wave", pool.dtype, (L,))])
        row["wave"][0] = pool[off : off + L]
        idx = np.flatnonzero(rid == r)
        mine = hits[idx].copy()
        mine["record_id"] = 0
        # one call per hit: the oracle drops rows silently, and the hit each kept row belongs to is needed for the order
        for i, h in zip(idx, mine):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # the mean of an empty record
                w = O.waveform_width(np.array([h]), row, **options)
            if len(w):
                w["record_id"] = r
                parts.append(w)
                order.append(i)
    if not parts:
        return np.zeros(0, dtype=WAVEFORM_WIDTH_DTYPE)
    return np.concatenate(parts)[np.argsort(np.asarray(order), kind="stable")]
