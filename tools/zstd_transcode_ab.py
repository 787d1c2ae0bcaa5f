#!/usr/bin/env python3
"""`cloudini_batch_transcode --compression zstd --device-zstd` against the same command without the flag (the method of
tools/sweep_transcode_ab.py): alternating fresh processes, one warm-up each, median (min .. max) of seconds_total over the
repetitions, output bytes side by side. An optional second executable (the parent commit's build) runs the plain command in
the same rotation: `zstd_transcode_ab.py [reps] [other_exe]`."""
import json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cloudini_amd import synth

EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
other = sys.argv[2] if len(sys.argv) > 2 else None
n_msgs = 256
KINDS = {"plain": (EXE, []), "device-zstd": (EXE, ["--device-zstd"])}
if other:
    KINDS["parent plain"] = (other, [])
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    distinct = [synth.velodyne_xyzir(130048, seed=42 + k) for k in range(4)]
    for k in range(n_msgs):
        info, data = distinct[k % 4]
        synth.cdr_pointcloud2(info, data, stamp=(1700000000, k)).tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    times = {kind: [] for kind in KINDS}
    stats = {}
    for r in range(reps + 1):
        for kind, (exe, extra) in KINDS.items():
            dst = os.path.join(tmp, "out_" + kind.replace(" ", "_"))
            p = subprocess.run([exe, src, dst, "--batch", "32", "--compression", "zstd"] + extra, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stdout + p.stderr
            stats[kind] = json.loads(p.stdout.strip().splitlines()[-1])
            if r:
                times[kind].append(stats[kind]["seconds_total"])
    line = f"{n_msgs} x 130048 Velodyne, batch 32, compression ZSTD, {reps} repetitions"
    for kind in KINDS:
        t, st = times[kind], stats[kind]
        line += (f"; {kind} median {statistics.median(t):.3f} s ({min(t):.3f} .. {max(t):.3f}), {st['points'] / statistics.median(t) / 1e6:.0f} Mpoints/s, "
                 f"seconds_gpu {st['seconds_gpu']:.3f}, seconds_stage2 {st['seconds_stage2']:.3f}, output {st['output_bytes']} B")
    line += f"; output bytes device-zstd / plain = {stats['device-zstd']['output_bytes'] / stats['plain']['output_bytes']:.4f}"
    print(line)
