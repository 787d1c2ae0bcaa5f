#!/usr/bin/env python3
"""`cloudini_batch_transcode --sweep ... --estimate` against the same command without --estimate and without either (the method
of tools/sweep_transcode_ab.py): alternating fresh processes, one warm-up each, median (min .. max) of seconds_total over the
repetitions; the outputs are compared file for file. ZSTD output: the `own` line then carries estimate / actual."""
import json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cloudini_amd import synth

EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
SWEEP = "xyz:0.0005,0.001,0.002,0.005; intensity:0.05,0.1,1"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_msgs = 256
KINDS = {"plain": [], "sweep": ["--sweep", SWEEP], "estimate": ["--sweep", SWEEP, "--estimate"]}
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    distinct = [synth.velodyne_xyzir(130048, seed=42 + k) for k in range(4)]
    for k in range(n_msgs):
        info, data = distinct[k % 4]
        synth.cdr_pointcloud2(info, data, stamp=(1700000000, k)).tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    times = {kind: [] for kind in KINDS}
    last = {}
    for r in range(reps + 1):
        for kind, extra in KINDS.items():
            dst = os.path.join(tmp, f"out_{kind}")
            p = subprocess.run([EXE, src, dst, "--batch", "32"] + extra, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stdout + p.stderr
            last[kind] = p.stdout
            if r:
                times[kind].append(json.loads(p.stdout.strip().splitlines()[-1])["seconds_total"])
    names = sorted(os.listdir(os.path.join(tmp, "out_plain")))
    same = all(open(os.path.join(tmp, "out_plain", f), "rb").read() == open(os.path.join(tmp, f"out_{kind}", f), "rb").read()
               for f in names for kind in ("sweep", "estimate"))
    line = f"{n_msgs} x 130048 Velodyne, batch 32, compression ZSTD, --sweep \"{SWEEP}\", {reps} repetitions, outputs identical: {same}"
    for kind in KINDS:
        t = times[kind]
        line += f"; {kind} median {statistics.median(t):.3f} s ({min(t):.3f} .. {max(t):.3f})"
    print(line)
    print("\n".join(ln for ln in last["estimate"].splitlines() if ln.startswith("estimate ")))
