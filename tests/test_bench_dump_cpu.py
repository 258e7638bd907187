"""bench.py --dump-outputs on CPU: the device is the stand-in of tests/bench_stub.py, so what is under test is bench.py's own
part -- the rows of the last timed step reach DIR as float32 / float64 arrays in canonical order, within the size budget,
the same on every run; --steps sets the number of timed steps; a larger table is cut to a seeded sample of whole records."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _bench(*extra):
    env = dict(os.environ, WFA_BENCH_STUB="tests.bench_stub", PYTHONPATH=REPO)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--records", "2000", "--no-features",
           "--no-cpu-baseline", *extra]
    return subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_last_step_rows(tmp_path):
    from tests.bench_stub import Session
    from waveformanalysis_amd.dtypes import THRESHOLD_HIT_DTYPE

    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        p = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert d["dump_outputs"]["rows"] == 1000 and d["dump_outputs"]["sampled"] is False
        runs.append(_load(out))
    a, b = runs
    assert sorted(a) == sorted(["hit_threshold_n"] + [f"hit_threshold_{f}" for f in THRESHOLD_HIT_DTYPE.names])
    assert sum(os.path.getsize(tmp_path / "run0" / f"{k}.npy") for k in a) <= 64_000_000
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k                  # identical inputs -> identical dump
    assert a["hit_threshold_n"].tolist() == [1000.0]
    from waveformanalysis_amd import synth

    s = Session()
    s.upload_records(synth.make_run(2000, "v1725", cfg=100)[0], 10.0)   # bench's rank-0 chunk
    want = s._fill_hits(s.hits_wait())
    want = want[np.argsort(want["record_id"], kind="stable")]  # canonical order: by record first
    for f in THRESHOLD_HIT_DTYPE.names:
        np.testing.assert_array_equal(a[f"hit_threshold_{f}"], want[f].astype(a[f"hit_threshold_{f}"].dtype), err_msg=f)


def test_steps_below_one_are_rejected():
    p = _bench("--steps", "0")
    assert p.returncode != 0 and "--steps" in p.stderr


def test_oversized_table_is_a_seeded_sample_of_whole_records(tmp_path):
    import bench
    from waveformanalysis_amd.dtypes import THRESHOLD_HIT_DTYPE

    rng = np.random.default_rng(3)
    n_rec = 5000
    per = rng.integers(0, 5, n_rec)
    rows = np.zeros(int(per.sum()), dtype=THRESHOLD_HIT_DTYPE)
    rows["record_id"] = np.repeat(np.arange(n_rec), per)
    rows["position"] = rng.integers(0, 800, len(rows))
    rows["height"] = rng.normal(size=len(rows))
    budget = 300_000
    first = bench.dump_hit_rows(rows, np.arange(n_rec), str(tmp_path / "a"), budget=budget)
    again = bench.dump_hit_rows(rows[rng.permutation(len(rows))], np.arange(n_rec), str(tmp_path / "b"), budget=budget)
    assert first["sampled"] and 0 < first["rows_written"] < len(rows) and first["bytes"] <= budget
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k                  # order of arrival does not matter
    rid = a["hit_threshold_record_id"].astype(np.int64)
    assert np.all(np.diff(rid) >= 0)
    kept, counts = np.unique(rid, return_counts=True)
    assert np.array_equal(counts, per[kept])                  # every chosen record with all of its rows
    assert a["hit_threshold_n"].tolist() == [float(len(rows))]
