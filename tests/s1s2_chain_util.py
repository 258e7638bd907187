"""Inputs and oracle tables of the S1/S2 peak chain tests: the two committed fixtures, a uniform synthetic run, and the
oracle chain hit -> waveform_width (per record) -> s1_s2 with basic_features on the side, computed once."""

from __future__ import annotations

import functools

import numpy as np

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import width_records_util as W

RAGGED_HIT = dict(height=8.0, prominence=0.5, width=2, distance=2)  # hit options of the ragged run
C5_RANGES = dict(s1_width_range=(0.0, 80.0), s2_width_range=(80.0, 5000.0), s1_area_range=None,
                 s2_area_range=(500.0, 1e12))  # the ranges of replay.c5_chain
OVERLAP = dict(s1_width_range=(0, 200), s2_width_range=(100, 5000), s1_height_range=(5, None))
# (class options, (unknown, S1, S2) the oracle gives on the ragged run)
RANGE_SETS = [
    (C5_RANGES, (0, 17, 9)),
    ({**OVERLAP, "conflict_policy": "unknown"}, (3, 17, 6)),
    ({**OVERLAP, "conflict_policy": "prefer_s1"}, (0, 20, 6)),
    ({**OVERLAP, "conflict_policy": "prefer_s2"}, (0, 17, 9)),
    (dict(width_unit="samples", s1_width_range=(0, 20), s2_width_range=(20, None)), (0, 17, 9)),
]


@functools.lru_cache(maxsize=None)
def run(name: str):
    """(records, wave_pool, hit options) of "positive" (32 uniform records), "ragged" (40 records of lengths 0 .. 1500)
    or "uniform" (256 x 800 samples, synthetic)."""
    if name == "positive":
        case = G.load_peaks("peaks_positive")
        return case["records"], case["wave_pool"], {}
    if name == "ragged":
        d = W.load()
        return d["records"], d["wave_pool"], RAGGED_HIT
    from waveformanalysis_amd import replay, synth

    rec, pool = replay.mirror_positive(*synth.make_run(256, "v1725", cfg=17))
    rec.setflags(write=False)
    pool.setflags(write=False)
    return rec, pool, {}


@functools.lru_cache(maxsize=None)
def oracle_tables(name: str, width_options_index: int = 0, width_filtered: bool = False):
    """(filtered pool, hit table, width rows, feature rows) of the oracle chain on a run."""
    rec, pool, hit_kw = run(name)
    filtered = O.filter_wave_pool(rec, pool)
    hits = O.find_peak_hits(rec, filtered, **hit_kw)
    options = W.load()["options"][width_options_index]
    widths = W.oracle_widths(hits, rec, filtered if width_filtered else pool, **options)
    return filtered, hits, widths, O.basic_features(rec, pool)


def oracle_rows(name: str, class_kw: dict, width_options_index: int = 0, width_filtered: bool = False) -> np.ndarray:
    _f, _h, widths, feats = oracle_tables(name, width_options_index, width_filtered)
    return O.s1_s2_classify(widths, feats, **class_kw)


def counts(rows: np.ndarray) -> tuple:
    return tuple(int(v) for v in np.bincount(rows["label"], minlength=3))
