"""Time k_waveform_width: its dense and its records instantiation on the same hits, and the plugin call on both routes.

Kernel leg: 125 000 x 800 samples, 250 000 hits (every record's maximum + one random position per record), int16 /
uint16 and float32.  The two instantiations alternate in one process, `--rounds` times each after one untimed pass;
kernel times are the HIP-event times of profile_report.  Prints the median, min and max per instantiation and checks
that both return the same rows.

End-to-end leg (`--e2e-records`, default 625 000 x 800 = 5e8 samples, positive twin of the synthetic run, one hit per
record at its maximum): wall time of HipWaveformWidthPlugin.compute on the dense route (st_waveforms: its rows are
uploaded and unpacked on the device by the first call and stay resident) and on the records route with the pool
resident; median of 3 after the call that uploads the samples, outputs compared.  `--e2e-records 0` skips it,
`--rounds 0` the kernel leg.  (tools/dense_time.py times the dense route against its host-copy form.)

One JSON line per leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformanalysis_amd import _lib, replay, synth  # noqa: E402
from waveformanalysis_amd.device import DeviceSession, default_pool  # noqa: E402
from waveformanalysis_amd.dtypes import HIT_DTYPE  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins import HipWaveformWidthPlugin  # noqa: E402


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def kernel_leg(rounds):
    n, L = 125000, 800
    rec, pool = synth.make_run(n, "v1725", cfg=7)
    pool = (16383 - pool.astype(np.int32)).clip(0, 16383).astype(np.uint16)   # positive pulses: the width plugin wants them
    rng = np.random.default_rng(1)
    pos = pool.reshape(n, L).argmax(axis=1).astype(np.int64)
    hits_pos = np.concatenate([pos, rng.integers(0, L, n)])
    hits_row = np.concatenate([np.arange(n), np.arange(n)]).astype(np.int64)
    with DeviceSession(0) as s:
        for name, p, src in (("int16", pool, _lib.SRC_RAW), ("float32", pool.astype(np.float32), _lib.SRC_F32)):
            s.upload_pool(p)
            s.upload_records(rec)   # offsets r * L: the records instantiation reads the very samples the dense one does
            calls = {"k_waveform_width": lambda: s.waveform_width(src, hits_pos, hits_row, n, L),
                     "k_waveform_width_rec": lambda: s.waveform_width_records(src, hits_pos, hits_row)}
            out = {k: call() for k, call in calls.items()}   # untimed
            ms = {k: [] for k in calls}
            for _ in range(rounds):
                for k, call in calls.items():
                    s.profile(True)
                    call()
                    (t, launches), = [v for kk, v in s.profile_report().items() if kk == k]
                    s.profile(False)
                    ms[k].append(t / launches)
            same = all(np.array_equal(out["k_waveform_width"][i], out["k_waveform_width_rec"][i]) for i in (0, 1))
            print(json.dumps({"leg": "kernel", "samples": name, "hits": len(hits_pos),
                              "valid": int(np.count_nonzero(out["k_waveform_width"][1])), "rounds": rounds,
                              "same_rows": bool(same), **{k: stats(v) for k, v in ms.items()}}), flush=True)


def e2e_leg(n_records):
    L = 800
    rec, pool = replay.mirror_positive(*synth.make_run(n_records, "v1725", cfg=7))
    hits = np.zeros(n_records, dtype=HIT_DTYPE)
    hits["position"] = pool.reshape(n_records, L).argmax(axis=1)
    for f in ("timestamp", "board", "channel", "record_id", "dt"):
        hits[f] = rec[f]
    st = replay.st_waveforms_from_records(rec, pool)
    plugin = HipWaveformWidthPlugin()
    routes = {"dense": SimpleContext({}, {"hit": hits, "st_waveforms": st}),
              "records": SimpleContext({"wave_source": "records"}, {"hit": hits, "records": rec, "wave_pool": pool})}
    result, out = {}, {}
    for name, ctx in routes.items():
        t0 = time.perf_counter()
        out[name] = plugin.compute(ctx, "run")   # the records route uploads the pool here, and only here
        first = time.perf_counter() - t0
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            again = plugin.compute(ctx, "run")
            wall.append(time.perf_counter() - t0)
            assert again.tobytes() == out[name].tobytes()
        result[name] = {"first_call_s": round(first, 4), "median_s": round(float(np.median(wall)), 4),
                        "min_s": round(min(wall), 4), "max_s": round(max(wall), 4)}
    sess = default_pool().session()
    print(json.dumps({"leg": "e2e", "n_records": n_records, "samples": n_records * L, "hits": len(hits),
                      "rows": len(out["dense"]), "same_rows": out["dense"].tobytes() == out["records"].tobytes(),
                      "pool_resident_after": bool(sess.holds_pool(pool)), "pool_uploads": sess.uploads, **result}),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--e2e-records", type=int, default=625000)
    args = ap.parse_args()
    if args.rounds:
        kernel_leg(args.rounds)
    if args.e2e_records:
        e2e_leg(args.e2e_records)
