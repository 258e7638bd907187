"""Time and host memory of the records stream against the static build of the same V1725 files.

Data: synthetic DAW_DEMO files written to a temporary directory -- `--files` files (default 4) whose events interleave
in time, 8 waves of `--samples` samples (default 1000) per event, the waves of an event 0..2 ticks out of order (so the
stream needs reorder_window_ns = 8 at dt = 4 ns).  Two run sizes a factor 4 apart: `--mib` MiB per file (default 16) and
four times that.  Ways, each in a fresh child process (peak resident memory is per process):

  static   records_builder.build_records_from_v1725_files: every file read whole, one sort, one gather;
  stream   HipRecordsStream.stream_files with `--block-mib` (default 8) per block, every chunk dropped once counted.

Per way: wall time, time to the first chunk (static: the end), resident memory before the run and at its peak
(ru_maxrss), and for the stream pushes, max_carry, max_carry_samples.  One more stream child per block size in
`--profile-block-mib` (default 8 and 64) runs the large run with the session's kernel timers on and reports the time of
the sample pass (k_rs_move) against the bytes it reads and writes (2 x 2 bytes per moved sample); one child times a
device-to-device copy of one block's size for comparison (torch, same accounting: bytes read + bytes written).  The files
have just been written, so reads come from the page cache for both ways.  Equality of the two ways is the tests' business
(tests/test_hip_records_stream.py); here the record and sample counts must agree.

    python tools/records_stream_time.py [--files 4] [--mib 16] [--samples 1000] [--block-mib 8] [--out PATH]
"""

from __future__ import annotations

import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

DT_NS = 4
WINDOW_NS = 8
CHANNELS = 8


def write_file(path: str, f: int, n_files: int, n_events: int, samples: int, seed: int) -> int:
    """One file of n_events events with mask 0x00FF; event e stands at tick (e * n_files + f) * 4000, its wave of channel k
    at + (2 - k % 3): inside the file a wave lies at most 2 ticks below the greatest timestamp before it."""
    rng = np.random.default_rng(seed)
    wave_bytes = 12 + 2 * samples
    event_bytes = 16 + CHANNELS * wave_bytes
    words = 3 + samples // 2
    per = 4096                                      # events per write
    with open(path, "wb") as fh:
        for e0 in range(0, n_events, per):
            n = min(per, n_events - e0)
            buf = np.zeros((n, event_bytes), dtype=np.uint8)
            buf[:, 4] = 0xFF
            base = (np.arange(e0, e0 + n, dtype=np.int64) * n_files + f) * 4000
            for k in range(CHANNELS):
                at = 16 + k * wave_bytes
                buf[:, at:at + 3] = np.frombuffer(int(words).to_bytes(3, "little"), dtype=np.uint8)
                ts = base + (2 - k % 3)
                buf[:, at + 4:at + 10] = ts.astype("<i8").view(np.uint8).reshape(n, 8)[:, :6]
                buf[:, at + 10:at + 12] = np.frombuffer(int(8000 + k).to_bytes(2, "little"), dtype=np.uint8)
                payload = rng.integers(7000, 9000, (n, samples), dtype=np.int16)
                buf[:, at + 12:at + wave_bytes] = payload.view(np.uint8)
            fh.write(buf.tobytes())
    return n_events * event_bytes


def rss_mib() -> float:
    with open("/proc/self/statm") as fh:
        return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2**20


def peak_mib() -> float:
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def child(args) -> None:
    paths = sorted(os.path.join(args.dir, n) for n in os.listdir(args.dir))
    out: dict = {"way": args.child}
    if args.child == "copy":
        import torch

        n = args.block_mib << 20
        a = torch.empty(n, dtype=torch.uint8, device="cuda").random_(0, 255)
        b = torch.empty_like(a)
        for _ in range(3):
            b.copy_(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        e0.record()
        for _ in range(reps):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        out.update(bytes=n, ms=ms, GBps_read_plus_write=2 * n / ms / 1e6)
        print(json.dumps(out))
        return
    from waveformanalysis_amd.device import default_pool
    from waveformanalysis_amd.records_builder import build_records_from_v1725_files
    from waveformanalysis_amd.records_stream import HipRecordsStream

    with default_pool().borrow() as sess:       # the device is up before the clock starts
        sess.sync()
    out["rss_before_mib"] = rss_mib()
    t0 = time.perf_counter()
    if args.child == "static":
        bundle = build_records_from_v1725_files(paths, dt_ns=DT_NS)
        t1 = time.perf_counter()
        out.update(records=len(bundle.records), samples=len(bundle.wave_pool), first_chunk_s=t1 - t0)
    else:
        stream = HipRecordsStream(block_bytes=args.block_mib << 20, reorder_window_ns=WINDOW_NS)
        stream.profile_pushes = bool(args.profile)
        first: list = []
        records = samples = chunks = 0
        for c in stream.stream_files(paths, DT_NS, first_chunk_time=first):
            records += len(c.data)
            samples += len(c.metadata["wave_pool"])
            chunks += 1
        t1 = time.perf_counter()
        st = dict(stream.stats)
        prof = st.pop("profile", None)
        out.update(records=records, samples=samples, chunks=chunks, first_chunk_s=(first[0] - t0) if first else None,
                   block_mib=args.block_mib, **st)
        if prof:
            ms, launches = prof.get("k_rs_move", (0.0, 0))
            moved = 4 * st["samples_moved"]      # 2 bytes read + 2 bytes written per sample
            out.update(move_ms=ms, move_launches=launches, move_bytes=moved,
                       move_GBps_read_plus_write=(moved / ms / 1e6) if ms else None,
                       other_ms={k: round(v[0], 3) for k, v in prof.items() if k != "k_rs_move"})
    out.update(wall_s=t1 - t0, rss_peak_mib=peak_mib())
    print(json.dumps(out))


def run_child(way: str, directory: str, block_mib: int, profile: bool = False) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", way, "--dir", directory, "--block-mib", str(block_mib)]
    if profile:
        cmd.append("--profile")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise RuntimeError(f"{way} child failed ({res.returncode}):\n{res.stderr[-2000:]}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--mib", type=int, default=16)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--block-mib", type=int, default=8)
    ap.add_argument("--profile-block-mib", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_stream_time.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    lines = [f"records stream vs static build: {args.files} V1725 files, {CHANNELS} waves of {args.samples} samples per event, "
             f"dt {DT_NS} ns, reorder_window_ns {WINDOW_NS}, stream block {args.block_mib} MiB"]
    event_bytes = 16 + CHANNELS * (12 + 2 * args.samples)
    results = []
    for scale in (1, 4):
        with tempfile.TemporaryDirectory() as d:
            n_events = (args.mib * scale << 20) // event_bytes
            total = sum(write_file(os.path.join(d, f"run_b{f % 2}_seg{f}.bin"), f, args.files, n_events, args.samples, 100 + f)
                        for f in range(args.files))
            lines.append(f"\nrun of {total / 2**20:.0f} MiB ({args.files} x {n_events} events, {args.files * n_events * CHANNELS} waves)")
            rows = [run_child("static", d, args.block_mib), run_child("stream", d, args.block_mib)]
            if rows[0]["records"] != rows[1]["records"] or rows[0]["samples"] != rows[1]["samples"]:
                raise RuntimeError(f"the ways disagree: {rows}")
            if scale == 4:
                rows += [run_child("stream", d, b, profile=True) for b in args.profile_block_mib]
            for r in rows:
                r["run_mib"] = total / 2**20
                results.append(r)
                tag = r["way"] + (f" block {r['block_mib']} MiB" if r["way"] == "stream" else "") + (" (timers on)" if "move_ms" in r else "")
                lines.append(f"  {tag:34s} wall {r['wall_s']:7.3f} s  first chunk {r['first_chunk_s']:7.3f} s  "
                             f"rss before {r['rss_before_mib']:7.0f} MiB  peak {r['rss_peak_mib']:7.0f} MiB")
                if r["way"] == "stream":
                    lines.append(f"  {'':34s} pushes {r['pushes']}  chunks {r['chunks']}  max_carry {r['max_carry']}  "
                                 f"max_carry_samples {r['max_carry_samples']}  bytes_read {r['bytes_read']}")
                if "move_ms" in r:
                    lines.append(f"  {'':34s} k_rs_move: {r['move_launches']} launches, {r['move_ms']:.3f} ms for "
                                 f"{r['move_bytes'] / 2**20:.0f} MiB read + written = {r['move_GBps_read_plus_write']:.0f} GB/s; "
                                 f"other device work of the pushes (ms): {r['other_ms']}")
    lines.append("")
    for b in args.profile_block_mib:
        with tempfile.TemporaryDirectory() as d:
            r = run_child("copy", d, b)
        results.append(r)
        lines.append(f"device-to-device copy of {b} MiB: {r['ms'] * 1000:.1f} us = {r['GBps_read_plus_write']:.0f} GB/s read + written")
    lines.append("\nJSON: " + json.dumps(results))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
