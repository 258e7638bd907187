"""bench.py --dump-outputs on the device: what lands in DIR is the hit table of the timed path -- the oracle's rows of the
same seeded chunk (bench's rank-0 inputs), integer fields bit-exact, in the dump's canonical order."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_dumped_rows_are_the_oracle_rows(tmp_path):
    import bench
    from oracle import wfa_oracle as O
    from waveformanalysis_amd import synth

    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--records", "4000",
           "--preheat-steps", "5", "--no-features", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)]
    proc = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    d = json.loads([ln for ln in proc.stdout.splitlines() if ln.strip()][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0

    rec, pool = synth.make_run(4000, "v1725", cfg=100)
    want = O.threshold_hits_chunked(rec, O.filter_wave_pool(rec, pool))
    want = want[np.lexsort([want[f] for f in reversed(bench.DUMP_ORDER)])]
    assert d["dump_outputs"]["rows"] == len(want) > 0 and d["dump_outputs"]["sampled"] is False
    assert np.load(tmp_path / "hit_threshold_n.npy").tolist() == [float(len(want))]
    for f in want.dtype.names:
        got = np.load(tmp_path / f"hit_threshold_{f}.npy")
        if want.dtype[f].kind in "iu":
            assert got.dtype == np.float64 and np.array_equal(got, want[f].astype(np.float64)), f
        else:
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, want[f], rtol=1e-6, err_msg=f)
