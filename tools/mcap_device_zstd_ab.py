#!/usr/bin/env python3
"""Same-box A/B of the bag converter's default path: another commit's build with `--mcap-compression zstd` (one host core
compresses every 2 MiB chunk) against this build with `--mcap-device-zstd` and with `--device-zstd-matches` on top.

  tools/mcap_device_zstd_ab.py <parent build dir> <this build dir> [--reps 5] [--workload NAME ...]

Build dirs, the installation of a build's libraries before every run and the workloads are tools/decode_transcode_ab.py's (the
256-message Velodyne bag, the 16-message depth-camera bag); the bags are written once into /dev/shm with tests/mcap_py.py.
Every run is a fresh process; the configurations alternate after one warm-up run each. Printed per run: seconds_total and the
mcap_* counters; per configuration the median and the spread (min .. max) of seconds_total and the size of the output file."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import decode_transcode_ab as AB  # noqa: E402
import mcap_py  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs=2, help="the parent commit's build, this build")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workload", nargs="*", default=list(AB.WORKLOADS))
    a = ap.parse_args()
    parent, this = (os.path.abspath(b) for b in a.builds)
    with tempfile.TemporaryDirectory() as keep:
        if os.path.samefile(this, AB.LIBDIR):
            for f in AB.LIBS + ("cloudini_batch_transcode",):
                shutil.copy2(os.path.join(this, f), os.path.join(keep, f))
            this = keep
        try:
            _measure(a, parent, this)
        finally:
            AB._install(this)


def _measure(a, parent, this):
    configs = [("P", "parent, --mcap-compression zstd", parent, []), ("T", "this build, --mcap-compression zstd", this, []),
               ("S", "this build --mcap-device-zstd", this, ["--mcap-device-zstd"]),
               ("M", "this build --mcap-device-zstd --device-zstd-matches", this, ["--mcap-device-zstd", "--device-zstd-matches"])]
    pc2 = "sensor_msgs/msg/PointCloud2"
    for name in a.workload:
        msgs, res, batch = AB.WORKLOADS[name]()
        with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
            src = os.path.join(tmp, "in.mcap")
            mcap_py.write(src, "ros2", [(1, pc2, "ros2msg", b"")], [(1, 1, "/points", "cdr", [])],
                          [(1, k, 1000 + k, 1000 + k, m.tobytes()) for k, m in enumerate(msgs)], chunk_messages=1)
            outs = [os.path.join(tmp, f"out_{c[0]}.mcap") for c in configs]
            args = lambda o, flags: [src, o, "--resolution", str(res), "--mcap-compression", "zstd", "--batch", str(batch)] + flags
            for (_tag, _label, build, flags), o in zip(configs, outs):
                AB._tool(build, args(o, flags))
            print(f"== {name}, batch {batch}: {len(msgs)} messages, input {os.path.getsize(src)} bytes", flush=True)
            totals = [[] for _ in configs]
            for rep in range(a.reps):
                for i, ((tag, _label, build, flags), o) in enumerate(zip(configs, outs)):
                    st = AB._tool(build, args(o, flags))
                    totals[i].append(st["seconds_total"])
                    print(f"   rep {rep} {tag}: seconds_total {st['seconds_total']:.4f} device chunks {st.get('mcap_device_chunks', '-')} "
                          f"device messages {st.get('mcap_device_messages', '-')} fallback {st.get('mcap_host_fallback_messages', '-')}", flush=True)
            for i, (tag, label, _build, _flags) in enumerate(configs):
                t = totals[i]
                print(f"   {tag} = {label}: seconds_total median {statistics.median(t):.4f}, spread {min(t):.4f} .. {max(t):.4f}; "
                      f"output {os.path.getsize(outs[i])} bytes", flush=True)
            med = [statistics.median(t) for t in totals]
            print(f"   S / P (medians) = {med[2] / med[0]:.2f}, M / P = {med[3] / med[0]:.2f}, T / P = {med[1] / med[0]:.2f}; "
                  f"size S / P = {os.path.getsize(outs[2]) / os.path.getsize(outs[0]):.4f}, M / P = {os.path.getsize(outs[3]) / os.path.getsize(outs[0]):.4f}",
                  flush=True)


if __name__ == "__main__":
    main()
