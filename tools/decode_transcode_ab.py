#!/usr/bin/env python3
"""Same-box A/B/C of the `--decode` transcode: another commit's build, this build, and this build with `--device-stage2`.

  tools/decode_transcode_ab.py <parent build dir> <this build dir> [--reps 5] [--compression lz4 zstd] [--threads 4 16]
                               [--workload NAME ...]

A build dir holds cloudini_batch_transcode next to its two libraries (cloudini_amd/lib, or a copy of another commit's). The
tool and libcloudini_amd.so name their libraries by the path they were linked at -- this tree's cloudini_amd/lib -- so a copy
elsewhere would load THIS build's libraries: before every run the build's two libraries are installed there (this build's own
are kept aside and put back at the end). The
input of every measured run is a directory of CompressedPointCloud2 messages in /dev/shm, written once per workload and
compression by this build's tool (host stage 2: libzstd level 1 / liblz4, the reference's bytes). Every run is a fresh process;
the three configurations alternate (P T D P T D ..., or as --order says) after one warm-up run each, with CLOUDINI_AMD_STAGE2_THREADS set to each
value of --threads. Printed per run: seconds_total, seconds_gpu and the stage-2 counters; per configuration the median and the
spread (min .. max) of seconds_total; and whether all three wrote the same files."""
import argparse
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cloudini_amd import synth  # noqa: E402


def _velodyne():
    distinct = [synth.velodyne_xyzir(130048, seed=42 + k) for k in range(4)]
    return [synth.cdr_pointcloud2(*distinct[k % 4], stamp=(1700000000, k)) for k in range(256)], 0.001, 32


def _depthcam():
    distinct = [synth.depthcam_xyzrgba(1280, 800, seed=42 + k) for k in range(2)]
    return [synth.cdr_pointcloud2(*distinct[k % 2], stamp=(1700000000, k)) for k in range(16)], 0.001, 8


WORKLOADS = {"velodyne_256x130048": _velodyne, "depthcam_16x1280x800": _depthcam}


LIBDIR = os.path.join(ROOT, "cloudini_amd", "lib")
LIBS = ("libcloudini_hip.so", "libcloudini_amd.so")
_installed = [None]


def _install(build):
    """the build's libraries at the path every copy of the tool loads them from"""
    if _installed[0] != build:
        for lib in LIBS:
            shutil.copyfile(os.path.join(build, lib), os.path.join(LIBDIR, lib + ".tmp"))
            os.replace(os.path.join(LIBDIR, lib + ".tmp"), os.path.join(LIBDIR, lib))
        _installed[0] = build


def _tool(build, args, threads=None):
    _install(build)
    exe = os.path.join(build, "cloudini_batch_transcode")
    env = dict(os.environ)
    if threads is not None:
        env["CLOUDINI_AMD_STAGE2_THREADS"] = str(threads)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        raise SystemExit(f"{exe} {' '.join(args)} failed: {r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs=2, help="the parent commit's build, this build")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compression", nargs="*", default=["lz4", "zstd"])
    ap.add_argument("--threads", nargs="*", type=int, default=[4, 16])
    ap.add_argument("--workload", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--order", default="PTD", help="the configurations to run and their order within a repetition")
    a = ap.parse_args()
    parent, this = (os.path.abspath(b) for b in a.builds)
    with tempfile.TemporaryDirectory() as keep:
        if os.path.samefile(this, LIBDIR):   # this build's files are about to be overwritten where they lie: measure a copy
            for f in LIBS + ("cloudini_batch_transcode",):
                shutil.copy2(os.path.join(this, f), os.path.join(keep, f))
            this = keep
        try:
            _measure(a, parent, this)
        finally:
            _install(this)


def _measure(a, parent, this):
    configs = [("P", "parent", parent, []), ("T", "this build", this, []), ("D", "this build --device-stage2", this, ["--device-stage2"])]
    configs = [next(c for c in configs if c[0] == tag) for tag in a.order]
    for name in a.workload:
        msgs, res, batch = WORKLOADS[name]()
        with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
            plain = os.path.join(tmp, "plain")
            os.makedirs(plain)
            for k, m in enumerate(msgs):
                m.tofile(os.path.join(plain, f"msg_{k:05d}.bin"))
            points = None
            for comp in a.compression:
                src = os.path.join(tmp, "in_" + comp)
                st = _tool(this, [plain, src, "--resolution", str(res), "--compression", comp, "--batch", str(batch)])
                points = st["points"]
                in_bytes = sum(os.path.getsize(os.path.join(src, f)) for f in os.listdir(src))
                for threads in a.threads:
                    outs = [os.path.join(tmp, f"out_{comp}_{threads}_{c[0]}") for c in configs]
                    for (_tag, _label, build, flags), o in zip(configs, outs):   # warm-up (and the files that are compared)
                        _tool(build, [src, o, "--decode", "--batch", str(batch)] + flags, threads)
                    same = True
                    for o in outs[1:]:
                        _m, mismatch, errors = filecmp.cmpfiles(outs[0], o, sorted(os.listdir(outs[0])), shallow=False)
                        same = same and not mismatch and not errors and sorted(os.listdir(outs[0])) == sorted(os.listdir(o))
                    print(f"== {name}, {comp}, batch {batch}, CLOUDINI_AMD_STAGE2_THREADS={threads}: {len(msgs)} messages, {points} points, "
                          f"{in_bytes} compressed bytes, outputs {'identical file for file' if same else 'DIFFER'}", flush=True)
                    totals = [[] for _ in configs]
                    for rep in range(a.reps):
                        for i, ((tag, _label, build, flags), o) in enumerate(zip(configs, outs)):
                            st = _tool(build, [src, o, "--decode", "--batch", str(batch)] + flags, threads)
                            totals[i].append(st["seconds_total"])
                            print(f"   rep {rep} {tag}: seconds_total {st['seconds_total']:.4f} seconds_gpu {st['seconds_gpu']:.4f} "
                                  f"gpu_batches {st['gpu_batches']} device_stage2_chunks {st.get('device_stage2_chunks', '-')} "
                                  f"host_stage2_chunks {st.get('host_stage2_chunks', '-')} retries {st.get('device_stage2_retries', '-')}", flush=True)
                    for i, (tag, label, _build, _flags) in enumerate(configs):
                        t = totals[i]
                        print(f"   {tag} = {label}: seconds_total median {statistics.median(t):.4f}, spread {min(t):.4f} .. {max(t):.4f}, "
                              f"{points / statistics.median(t) / 1e6:.1f} Mpoints/s", flush=True)
                    med = {c[0]: statistics.median(t) for c, t in zip(configs, totals)}
                    if "D" in med and "T" in med:
                        print(f"   D / T (medians) = {med['D'] / med['T']:.2f}", flush=True)
                    if "T" in med and "P" in med:
                        print(f"   T / P (medians) = {med['T'] / med['P']:.2f}", flush=True)


if __name__ == "__main__":
    main()
