#!/usr/bin/env python3
"""`cloudini_batch_transcode --modes report` and `--modes best` against the same command without the option (the method of
tools/sweep_transcode_ab.py): alternating fresh processes, one warm-up each, median (min .. max) of seconds_total over the
repetitions. Every fourth message has a ring column that fools the probe (constant over the first 4096 points, noise behind
them), so `best` has runs to encode again; the report run's outputs are compared file for file with the plain run's."""
import json, os, statistics, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cloudini_amd import synth

EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n_msgs = 256
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    distinct = [synth.velodyne_xyzir(130048, seed=42 + k) for k in range(4)]
    info, data = distinct[3]
    ring = data.reshape(-1, info.point_step)[:, 16:18].view("<u2").reshape(-1)
    ring[:4096] = 9
    ring[4096:] = np.random.RandomState(3).randint(0, 1 << 15, ring.size - 4096)
    for k in range(n_msgs):
        info, data = distinct[k % 4]
        synth.cdr_pointcloud2(info, data, stamp=(1700000000, k)).tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    kinds = ("plain", "report", "best")
    times = {k: [] for k in kinds}
    last = {}
    for r in range(reps + 1):
        for kind in kinds:
            dst = os.path.join(tmp, f"out_{kind}")
            cmd = [EXE, src, dst, "--compression", "none", "--batch", "32"] + ([] if kind == "plain" else ["--modes", kind])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stdout + p.stderr
            last[kind] = p.stdout
            if r:
                times[kind].append(json.loads(p.stdout.strip().splitlines()[-1])["seconds_total"])
    names = sorted(os.listdir(os.path.join(tmp, "out_plain")))
    same = all(open(os.path.join(tmp, "out_plain", f), "rb").read() == open(os.path.join(tmp, "out_report", f), "rb").read() for f in names)
    size = {k: sum(os.path.getsize(os.path.join(tmp, f"out_{k}", f)) for f in names) for k in kinds}
    line = f"{n_msgs} x 130048 Velodyne (every 4th fools the probe), batch 32, compression none, {reps} repetitions, report outputs identical: {same}"
    for kind in kinds:
        t = times[kind]
        line += f"; {kind} median {statistics.median(t):.3f} s ({min(t):.3f} .. {max(t):.3f})"
    print(line)
    print(f"output bytes: plain {size['plain']}, best {size['best']} (saved {size['plain'] - size['best']})")
    print("\n".join(ln for ln in last["best"].splitlines() if ln.startswith("modes ")))
