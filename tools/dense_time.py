"""Time the dense route on one st_waveforms array: the upload alone and the five-plugin chain hit_threshold ->
basic_features -> waveform_width_integral -> hit -> waveform_width, with the rows unpacked on the device and resident
(DeviceSession.dense_rows = True) and on the host route (False: a contiguous host copy of `wave` uploaded by every plugin).

Input: `--records` x 800 samples (default 625 000 = 5e8 samples), the positive twin of the synthetic V1725 run.

Upload leg, per route, median / min / max of 3: wall time of putting the samples on the device (rows: upload_dense of the
array as it is; host: dense.dense_pool + upload_pool) and the rate of the last staged copy (wfa_last_h2d_rate; for the
rows route that is one batch of DENSE_BATCH_BYTES).
Chain leg, per route: the chain once from an empty session (`first_s`), then 3 more times in new contexts over the same
array (`repeat_s`), each with its pool uploads; the tables of the two routes are compared byte for byte.
`--upload-only` stops after the upload leg (what a `rocprofv3 --kernel-trace --stats` run of k_dense_unpack needs).

One JSON line per leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformanalysis_amd import dense, replay, synth  # noqa: E402
from waveformanalysis_amd.device import DeviceSession, default_pool  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins import (  # noqa: E402
    HipBasicFeaturesPlugin,
    HipHitFinderPlugin,
    HipThresholdHitPlugin,
    HipWaveformWidthIntegralPlugin,
    HipWaveformWidthPlugin,
)

CHAIN = ("hit_threshold", "basic_features", "waveform_width_integral", "hit", "waveform_width")
ROUTES = {"rows": True, "host": False}


def stats(s):
    return {"median_s": round(float(np.median(s)), 4), "min_s": round(min(s), 4), "max_s": round(max(s), 4)}


def upload_leg(st):
    sess = default_pool().session()
    out = {}
    for route in ROUTES:
        wall, rate = [], []
        for _ in range(4):  # the first one allocates the device buffers: not counted
            sess.forget_resident()
            t0 = time.perf_counter()
            if route == "rows":
                sess.upload_dense(st)
            else:
                sess.upload_pool(dense.dense_pool(st)[0])
            wall.append(time.perf_counter() - t0)
            rate.append(sess.last_h2d_rate())
        out[route] = {**stats(wall[1:]), "h2d_GBps": round(float(np.median(rate[1:])), 2)}
    nbytes = {"rows": st.nbytes, "host": st["wave"].size * 2}
    print(json.dumps({"leg": "upload", "rows": len(st), "samples": int(st["wave"].size), "bytes": nbytes, **out}), flush=True)


def chain(st, rec):
    ctx = SimpleContext({"hit": {"use_filtered": False}}, {"st_waveforms": st, "records": rec},
                        plugins=[HipThresholdHitPlugin(), HipBasicFeaturesPlugin(), HipWaveformWidthIntegralPlugin(),
                                 HipHitFinderPlugin(), HipWaveformWidthPlugin()])
    sess = default_pool().session()
    before, per_plugin, tables = sess.uploads, {}, {}
    t_all = time.perf_counter()
    for name in CHAIN:
        t0 = time.perf_counter()
        tables[name] = ctx.get_data("run", name)
        per_plugin[name] = round(time.perf_counter() - t0, 4)
    return tables, time.perf_counter() - t_all, sess.uploads - before, per_plugin


def chain_leg(st, rec):
    sess = default_pool().session()
    result, tables = {}, {}
    for route, switch in ROUTES.items():
        DeviceSession.dense_rows = switch
        sess.forget_resident()
        tables[route], first, first_uploads, first_plugins = chain(st, rec)
        wall, uploads, plugins = [], [], None
        for _ in range(3):
            again, t, u, plugins = chain(st, rec)
            wall.append(t)
            uploads.append(u)
            assert all(again[k].tobytes() == tables[route][k].tobytes() for k in CHAIN)
        result[route] = {"first_s": round(first, 4), "first_uploads": first_uploads, "first_plugins_s": first_plugins,
                         "repeat_s": stats(wall), "repeat_uploads": uploads, "repeat_plugins_s": plugins}
    DeviceSession.dense_rows = True
    same = all(tables["rows"][k].tobytes() == tables["host"][k].tobytes() for k in CHAIN)
    print(json.dumps({"leg": "chain", "rows": len(st), "samples": int(st["wave"].size),
                      "table_rows": {k: len(tables["rows"][k]) for k in CHAIN}, "same_tables": bool(same), **result}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=625000)
    ap.add_argument("--upload-only", action="store_true")
    args = ap.parse_args()
    rec, pool = replay.mirror_positive(*synth.make_run(args.records, "v1725", cfg=7))
    st = replay.st_waveforms_from_records(rec, pool)
    del pool
    upload_leg(st)
    if not args.upload_only:
        chain_leg(st, rec)
