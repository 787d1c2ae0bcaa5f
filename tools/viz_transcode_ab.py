#!/usr/bin/env python3
"""Same-box A/B of the `--viz` transcode between two library builds.

  tools/viz_transcode_ab.py <build dir A> <build dir B> [--reps 5] [--compression none|zstd] [--workload NAME ...]

A build dir holds cloudini_batch_transcode next to its two libraries (cloudini_amd/lib, or a copy of another commit's under
cloudini_amd/lib/variants/<name>/). Every run is a fresh process of that build's tool on a directory in /dev/shm; the builds
alternate (A B A B ...) after one warm-up run each. Printed per run: seconds_total, seconds_gpu, points; per build the median
and the spread (min .. max) of seconds_total; and whether the two builds wrote the same files.

seconds_gpu is NOT comparable across the change that moved the filter into the run's GPU call: before it the clock started
behind the per-message filter calls, now it covers the fused filter + encode call. The judged figure is seconds_total with
compression none (stage 2 is then a copy, the GPU stage is what is left)."""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cloudini_amd import synth  # noqa: E402


def _velodyne():
    distinct = [synth.velodyne_xyzir(130048, seed=42 + k) for k in range(4)]
    return [synth.cdr_pointcloud2(*distinct[k % 4], stamp=(1700000000, k)) for k in range(256)], 0.25, 32


def _depthcam(res):
    distinct = [synth.depthcam_xyzrgba(1280, 800, seed=42 + k) for k in range(2)]
    return [synth.cdr_pointcloud2(*distinct[k % 2], stamp=(1700000000, k)) for k in range(16)], res, 8


WORKLOADS = {
    "velodyne_256x130048_at_0.25": _velodyne,                    # 62 % survive
    "depthcam_16x1280x800_at_0.01": lambda: _depthcam(0.01),     # 16 % survive
    "depthcam_16x1280x800_at_0.001": lambda: _depthcam(0.001),   # 95 % survive: NaN drop only
}


def _run(build, src, dst, res, batch, compression):
    exe = os.path.join(build, "cloudini_batch_transcode")
    r = subprocess.run([exe, src, dst, "--resolution", str(res), "--compression", compression, "--viz", "--batch", str(batch)],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{exe} failed: {r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compression", default="none")
    ap.add_argument("--workload", nargs="*", default=list(WORKLOADS))
    a = ap.parse_args()
    builds = [os.path.abspath(b) for b in a.builds]
    for name in a.workload:
        msgs, res, batch = WORKLOADS[name]()
        with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
            src = os.path.join(tmp, "in")
            os.makedirs(src)
            for k, m in enumerate(msgs):
                m.tofile(os.path.join(src, f"msg_{k:05d}.bin"))
            outs = [os.path.join(tmp, "out_a"), os.path.join(tmp, "out_b")]
            for b, o in zip(builds, outs):
                _run(b, src, o, res, batch, a.compression)      # warm-up (and the files that are compared)
            _m, mismatch, errors = filecmp.cmpfiles(outs[0], outs[1], sorted(os.listdir(outs[0])), shallow=False)
            same = not mismatch and not errors and sorted(os.listdir(outs[0])) == sorted(os.listdir(outs[1]))
            print(f"== {name}, compression {a.compression}, batch {batch}: {len(msgs)} messages, outputs "
                  f"{'identical file for file' if same else 'DIFFER: ' + str((mismatch + errors)[:5])}", flush=True)
            totals = [[], []]
            for rep in range(a.reps):
                for i, (b, o) in enumerate(zip(builds, outs)):
                    st = _run(b, src, o, res, batch, a.compression)
                    totals[i].append(st["seconds_total"])
                    print(f"   rep {rep} {'AB'[i]}: seconds_total {st['seconds_total']:.4f} seconds_gpu {st['seconds_gpu']:.4f} "
                          f"points {st['points']} gpu_batches {st['gpu_batches']}", flush=True)
            for i, b in enumerate(builds):
                t = totals[i]
                print(f"   {'AB'[i]} = {os.path.relpath(b, ROOT)}: seconds_total median {statistics.median(t):.4f}, "
                      f"spread {min(t):.4f} .. {max(t):.4f}", flush=True)
            print(f"   A / B (medians) = {statistics.median(totals[0]) / statistics.median(totals[1]):.2f}", flush=True)


if __name__ == "__main__":
    main()
