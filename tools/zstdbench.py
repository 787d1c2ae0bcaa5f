#!/usr/bin/env python3
"""Device-side ZSTD (cloudini_amd/csrc/zstd_kernels.hip: frames of literal-only blocks) on device-resident batches:
32 x 1 M lidar_xyzi and 64 x 130048 velodyne_xyzir. One encode_device call per measurement, the modes interleaved
(stage 1 only, device ZSTD, device ZSTD with matches -- cldn_hip_codec_set_zstd_matches, zstd_seq_kernels.hip --, device LZ4,
device LZ4 FAST, round after round); median [min .. max] of the repetitions. The stage-2 part of a mode is its call minus the
stage-1-only call of the same round; the mode with matches is also held against the literal-only mode of the same round. Next to it what the host route has to do
for the same chunks once they are in host memory: ZSTD_compress(level 1) per chunk on 1 and 16 threads (the stage-2 pool's
work alone, no copies), and the sizes of all routes side by side.

`zstdbench.py once` runs one device-ZSTD call per batch and nothing else (for a kernel trace); `zstdbench.py once-matches` the
same with the matches switch on."""
import ctypes as C
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth

dev = torch.device("cuda", 0)
REPS = int(os.environ.get("ZSTDBENCH_REPS", "12")) if len(sys.argv) < 3 else int(sys.argv[2])
once = len(sys.argv) > 1 and sys.argv[1] in ("once", "once-matches")
ZSTD_MATCHES = 3 | 0x100   # a key of this script: stage 2 = 3 with set_zstd_matches(True)
MODES = [(0, "stage 1 only"), (3, "device ZSTD"), (ZSTD_MATCHES, "ZSTD + matches"), (1, "device LZ4"), (2, "device LZ4 FAST")]

z = C.CDLL("libzstd.so.1")
z.ZSTD_compress.restype = C.c_size_t
z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
z.ZSTD_compressBound.restype = C.c_size_t
z.ZSTD_compressBound.argtypes = [C.c_size_t]


def stat(t):
    return f"{np.median(t)*1e3:.3f} ms [{min(t)*1e3:.3f} .. {max(t)*1e3:.3f}]"


for wl, gen, n_clouds in (("lidar_xyzi 1M", lambda k: synth.lidar_xyzi(1_000_000, seed=7 + k), 32),
                          ("velodyne_xyzir 130048", lambda k: synth.velodyne_xyzir(130048, seed=42 + k), 64)):
    distinct = [gen(k) for k in range(4)]
    info = distinct[0][0]
    pts = distinct[0][1].size // info.point_step
    plan = native.Plan(info)
    codec = native.Codec(plan)
    d_in = torch.from_numpy(np.concatenate([distinct[k % 4][1] for k in range(n_clouds)])).to(dev)
    cp = np.full(n_clouds, pts, dtype=np.uint64)
    cap = max(plan.stage2_bound(pts, m & 0xff) for m, _ in MODES) * n_clouds
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n_clouds + 1, dtype=torch.int64, device=dev)

    def call(mode):
        codec.set_stage2(mode & 0xff)
        codec.set_zstd_matches(mode == ZSTD_MATCHES)
        t0 = time.perf_counter()
        codec.encode_device(d_in.data_ptr(), cp, d_out.data_ptr(), cap, d_off.data_ptr())
        codec.synchronize()
        return time.perf_counter() - t0

    if once:
        which = ZSTD_MATCHES if sys.argv[1] == "once-matches" else 3
        call(which)
        call(which)
        codec.status()
        print(f"{wl} x{n_clouds}: two device-ZSTD calls{' with matches' if which != 3 else ''}, {int(d_off.cpu()[-1])} bytes")
        codec.close()
        continue
    size = {}
    for mode, _ in MODES:
        for _ in range(3):
            call(mode)
        codec.status()
        size[mode] = int(d_off.cpu()[-1])
    times = {mode: [] for mode, _ in MODES}
    for _ in range(REPS):
        for mode, _ in MODES:
            times[mode].append(call(mode))
    codec.status()
    # the stage-1 streams of the batch in host memory: what the host pool compresses
    call(0)
    total = int(d_off.cpu()[-1])
    s1 = d_out[:total].cpu().numpy()
    chunks, o = [], 0
    while o < total:
        n = int.from_bytes(s1[o:o + 4].tobytes(), "little")
        chunks.append(s1[o + 4:o + 4 + n])
        o += 4 + n
    payload = sum(c.size for c in chunks)
    bound = z.ZSTD_compressBound(max(c.size for c in chunks))
    outs = [np.empty(bound, np.uint8) for _ in chunks]
    host_sizes = [0] * len(chunks)

    def one(k):
        host_sizes[k] = z.ZSTD_compress(outs[k].ctypes.data, bound, chunks[k].ctypes.data, chunks[k].size, 1)
    host = {}
    for threads in (1, 16):
        with ThreadPoolExecutor(threads) as ex:
            t = []
            for _ in range(max(3, REPS // 4)):
                t0 = time.perf_counter()
                list(ex.map(one, range(len(chunks))))
                t.append(time.perf_counter() - t0)
        host[threads] = t
    host_bytes = sum(host_sizes) + 4 * len(chunks)
    base = np.array(times[0])
    print(f"{wl} x{n_clouds} ({n_clouds * pts / 1e6:.1f} Mpoints, {len(chunks)} chunks, {payload / 1e6:.1f} MB of stage-1 payload), {REPS} interleaved repetitions")
    print(f"  stage 1 only      {stat(times[0])}  {size[0]} B")
    for mode, tag in MODES[1:]:
        part = np.array(times[mode]) - base
        print(f"  + {tag:15s} {stat(times[mode])}  {size[mode]} B ({size[mode] / size[0]:.4f} of stage 1) -> stage-2 part {stat(part)}, "
              f"{payload / np.median(part) / 1e9:.1f} GB/s of payload, {n_clouds * pts / np.median(times[mode]) / 1e6:.0f} Mpoints/s for the call")
    for threads in (1, 16):
        t = host[threads]
        print(f"  host ZSTD level 1, {threads:2d} thread(s) {stat(t)}  {host_bytes} B ({host_bytes / size[0]:.4f} of stage 1), "
              f"{payload / np.median(t) / 1e9:.2f} GB/s of payload")
    print(f"  size: device ZSTD / host ZSTD = {size[3] / host_bytes:.4f}; device ZSTD part / host 16 threads = "
          f"{np.median(np.array(times[3]) - base) / np.median(host[16]):.4f}")
    lit_part, seq_part = np.array(times[3]) - base, np.array(times[ZSTD_MATCHES]) - base
    print(f"  with matches: size / host ZSTD = {size[ZSTD_MATCHES] / host_bytes:.4f}, / literal-only = {size[ZSTD_MATCHES] / size[3]:.4f}; "
          f"stage-2 part / literal-only part of the same round = {np.median(seq_part / lit_part):.3f} "
          f"[{(seq_part / lit_part).min():.3f} .. {(seq_part / lit_part).max():.3f}]")
    codec.close()
