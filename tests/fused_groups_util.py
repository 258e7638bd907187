"""Shared by tests/test_hip_fused_groups.py and tests/test_fused_groups_cpu.py: the fixture
tests/golden/c5_fused_groups.npz, its configuration (as in tests/golden/make_fused_groups_golden.py, which imports the
reference and cannot be imported here) and the per-group passes of the merge tests."""

from __future__ import annotations

import functools
import os

import numpy as np

from tests.golden_util import GOLDEN
from waveformanalysis_amd import _lib
from waveformanalysis_amd.filter_engine import design_bw
from waveformanalysis_amd.plugin_api import SimpleContext

RUNS = ["a", "b", "c"]
FILTER_CC = {"0:1": {"sg_window_size": 7, "sg_poly_order": 3},
             "0:2": {"sg_window_size": 21, "sg_poly_order": 4},
             "0:3": {"filter_type": "BW", "lowcut": 0.01, "highcut": 0.2, "fs": 0.5}}
HIT_CC = {"0:1": {"threshold": 2.0}, "0:3": {"threshold": 3.0}}
# the resolved filter key of every channel, in the order the channels first appear in the records
KEYS = [("SG", 11, 2), ("SG", 7, 3), ("SG", 21, 4), ("BW", 0.01, 0.2, 0.5, 4)]
THRESHOLDS = [10.0, 2.0, 10.0, 3.0]


@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(os.path.join(GOLDEN, "c5_fused_groups.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def load_run(tag: str) -> dict:
    """{"records", "wave_pool", "wave_pool_filtered", "hits", "hits_uniform"} of one run (the arrays are shared between
    the tests: copy before writing)."""
    d = _fixture()
    return {name: d[f"{name}_{tag}"] for name in ("records", "wave_pool", "wave_pool_filtered", "hits", "hits_uniform")}


def context(run: dict, hit_cfg: dict, filter_cfg: dict, devices=None) -> SimpleContext:
    from waveformanalysis_amd.plugins import HipThresholdHitPlugin, HipWavePoolFilteredPlugin

    return SimpleContext({"wave_source": "records", "hit_threshold": dict(hit_cfg, devices=devices),
                          "wave_pool_filtered": dict(filter_cfg)},
                         {"records": run["records"], "wave_pool": run["wave_pool"]},
                         plugins=[HipWavePoolFilteredPlugin(), HipThresholdHitPlugin()])


def group_plan(records: np.ndarray) -> list[tuple[tuple, np.ndarray]]:
    """[(filter key, mask)] of FILTER_CC on `records`: channel c has KEYS[c]."""
    return [(key, records["channel"] == c) for c, key in enumerate(KEYS)]


def group_column(plan) -> np.ndarray:
    """group_of_record of a plan's masks: int32, the index of the record's group, -1 where no mask holds."""
    column = np.full(len(plan[0][1]), -1, dtype=np.int32)
    for g, (_key, mask) in enumerate(plan):
        column[mask] = g
    return column


def thresholds_of(records: np.ndarray) -> np.ndarray:
    """HIT_CC per record."""
    return np.asarray(THRESHOLDS)[records["channel"]]


def run_groups(sess, records: np.ndarray, thresholds: np.ndarray, plan) -> tuple[list[np.ndarray], int]:
    """Every group's single pass alone on a session that holds the pool, +inf outside the group, each downloaded; then
    the queued grouped call -> (the downloads in pass order, the row count of the device-merged table, left resident)."""
    for key, mask in plan:  # the Butterworth records into the float32 twin, before the table of the passes is uploaded
        if key[0] == "BW":
            sess.upload_records(records[mask])
            sess.sosfiltfilt(*design_bw(*key[1:]), download=False)
    parts = []
    for key, mask in plan:
        sess.upload_records(records, np.where(mask, thresholds, np.inf))
        if key[0] == "SG":
            sess.set_sg_plan(key[1], key[2])
            parts.append(sess.threshold_hits(_lib.SRC_SG_FUSED))
        else:
            parts.append(sess.threshold_hits(_lib.SRC_F32))
    sess.upload_records(records, thresholds)
    stage_groups(sess, [key for key, _mask in plan], group_column(plan))
    return parts, sess.hits_wait()


def stage_groups(sess, keys, group_of_record, baseline_window=(0, 0)) -> None:
    """The queued grouped pass over the uploaded records, group g in plan slot g; hits_wait() delivers."""
    groups = []
    for g, key in enumerate(keys):
        if key[0] == "BW":
            sess.sosfiltfilt_group(*design_bw(*key[1:]), group_of_record, g)
            groups.append((_lib.SRC_F32, 0))
        else:
            sess.store_sg_plan(g, key[1], key[2])
            groups.append((_lib.SRC_SG_FUSED, g))
    sess.hits_enqueue_groups(groups, group_of_record, 2, 2, baseline_window=baseline_window)


def host_merge(records: np.ndarray, parts: list[np.ndarray]) -> np.ndarray:
    """The downloads of the passes merged by record index (position of the row's record_id in the table), the rows of
    one record in pass order."""
    rows = np.concatenate(parts)
    ids = np.asarray(records["record_id"], dtype=np.int64)
    by_id = np.argsort(ids, kind="stable")
    index = by_id[np.searchsorted(ids[by_id], rows["record_id"])]
    return rows[np.argsort(index, kind="stable")]
