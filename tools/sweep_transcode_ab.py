#!/usr/bin/env python3
"""`cloudini_batch_transcode --sweep` against the same command without it (the method of tools/audit_transcode_ab.py):
alternating fresh processes, one warm-up each, median (min .. max) of seconds_total over the repetitions; the outputs are
compared file for file."""
import json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cloudini_amd import synth

EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
SWEEP = "xyz:0.0005,0.001,0.002,0.005; intensity:0.05,0.1,1"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_msgs = 256
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    distinct = [synth.velodyne_xyzir(130048, seed=42 + k) for k in range(4)]
    for k in range(n_msgs):
        info, data = distinct[k % 4]
        synth.cdr_pointcloud2(info, data, stamp=(1700000000, k)).tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    times = {"plain": [], "sweep": []}
    for r in range(reps + 1):
        for kind in ("plain", "sweep"):
            dst = os.path.join(tmp, f"out_{kind}")
            cmd = [EXE, src, dst, "--compression", "none", "--batch", "32"] + (["--sweep", SWEEP] if kind == "sweep" else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stdout + p.stderr
            if r:
                times[kind].append(json.loads(p.stdout.strip().splitlines()[-1])["seconds_total"])
    same = all(open(os.path.join(tmp, "out_plain", f), "rb").read() == open(os.path.join(tmp, "out_sweep", f), "rb").read()
               for f in sorted(os.listdir(os.path.join(tmp, "out_plain"))))
    line = f"{n_msgs} x 130048 Velodyne, batch 32, compression none, --sweep \"{SWEEP}\", {reps} repetitions, outputs identical: {same}"
    for kind in ("plain", "sweep"):
        t = times[kind]
        line += f"; {kind} median {statistics.median(t):.3f} s ({min(t):.3f} .. {max(t):.3f})"
    print(line)
