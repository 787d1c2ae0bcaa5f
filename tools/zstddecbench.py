#!/usr/bin/env python3
"""Device-side ZSTD decode (cloudini_amd/csrc/zstd_decode.hip) on clouds encoded with CLDN_HIP_STAGE2_ZSTD: 32 x 1 M lidar_xyzi
and 64 x 130048 velodyne_xyzir.

  resident   streams in HBM: decode_zstd_device against decode_device on the same clouds' stage-1 streams; the stage-2 part is
             the difference of the two calls OF THE SAME ROUND, as GB/s of decoded payload
  messages   the same clouds as ZSTD messages in host memory, one PointcloudDecoder::decode per message: the host route (libzstd
             on the stage-2 pool) with 1 and 16 threads, switch (set_device_zstd_decode) off and on
Interleaved: every round runs every variant once, in the same order; 3 warm-up rounds, then 12 measured: median [min .. max].
`zstddecbench.py once` makes the resident calls once each (for a kernel trace).
`zstddecbench.py seq [once]` measures frames WITH sequences instead (zstd_seq_decode.hip, cldn_hip_codec_set_zstd_sequences):
the same clouds' stage-1 chunks compressed by libzstd (level 1, what PointcloudEncoder writes), HBM-resident against the plain
stage-1 call, then as host messages: the host route on 1 and 16 threads against the device route with both switches on
(set_device_zstd_decode, set_device_zstd_sequences). The workloads, rounds and batch sizes are the same."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import api, native, synth
from cloudini_amd.schema import CompressionOption

dev = torch.device("cuda", 0)
ZSTD = 3
ONCE = "once" in sys.argv[1:]
SEQ = "seq" in sys.argv[1:]
WARM, REPS = (0, 1) if ONCE else (3, 12)


def fmt(t):
    t = np.asarray(t)
    return f"{np.median(t)*1e3:.3f} ms [{t.min()*1e3:.3f} .. {t.max()*1e3:.3f}]"


def one(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


for wl, gen, n_clouds in (("lidar_xyzi 1M", lambda: synth.lidar_xyzi(1_000_000), 32),
                          ("velodyne_xyzir 130048", lambda: synth.velodyne_xyzir(130048), 64)):
    info, data = gen()
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    pts = data.size // info.point_step
    plan = native.Plan(info)
    codec = native.Codec(plan)
    cp = np.full(n_clouds, pts, dtype=np.uint64)
    s1 = codec.encode_host([data])[0][0]
    codec.set_stage2(ZSTD)
    frames = codec.encode_host([data])[0][0]
    codec.set_stage2(0)
    if SEQ:  # libzstd's frames of the same chunks: the body of a host message
        zi = info.copy(compression_opt=CompressionOption.ZSTD, use_threads=True)
        e = api.PointcloudEncoder(zi)
        frames = np.ascontiguousarray(e.encode(data)[len(e.getHeader()):])
        codec.set_zstd_sequences(True)
    d_pts = torch.zeros(data.size * n_clouds, dtype=torch.uint8, device=dev)

    def resident(stream):
        d = torch.from_numpy(np.concatenate([stream] * n_clouds)).to(dev)
        return d, np.arange(n_clouds + 1, dtype=np.uint64) * np.uint64(stream.size)
    d_s1, o_s1 = resident(s1)
    d_z, o_z = resident(frames)
    payload = (s1.size - 4 * ((pts + 32767) // 32768)) * n_clouds
    variants = {
        "stage-1 streams": lambda: codec.decode_device(d_s1.data_ptr(), o_s1, cp, d_pts.data_ptr(), d_pts.numel()),
        "ZSTD frames": lambda: codec.decode_zstd_device(d_z.data_ptr(), o_z, cp, d_pts.data_ptr(), d_pts.numel()),
    }
    times = {k: [] for k in variants}
    for r in range(WARM + REPS):
        for k, fn in variants.items():
            t = one(fn, codec.synchronize)
            if r >= WARM:
                times[k].append(t)
    codec.status()
    part = np.asarray(times["ZSTD frames"]) - np.asarray(times["stage-1 streams"])
    print(f"decode {wl} x{n_clouds}, HBM-resident: stage-1 streams {fmt(times['stage-1 streams'])} ({payload/1e6:.1f} MB of payload)")
    print(f"decode {wl} x{n_clouds}, HBM-resident: {'libzstd' if SEQ else 'device'} ZSTD frames ({frames.size*n_clouds/1e6:.1f} MB) {fmt(times['ZSTD frames'])} -> "
          f"ZSTD part {fmt(part)}, {payload/np.median(part)/1e9:.2f} GB/s of decoded payload")
    codec.close()
    if ONCE:
        continue
    # the same clouds as ZSTD messages in host memory
    zinfo = info.copy(compression_opt=CompressionOption.ZSTD, use_threads=True)
    enc = api.PointcloudEncoder(zinfo)
    hdr = len(enc.getHeader())
    bodies = {"libzstd": np.ascontiguousarray(enc.encode(data)[hdr:]), "device frames": np.ascontiguousarray(frames)}
    if SEQ:
        del bodies["device frames"]
    L = api.lib()
    ci, _keep = api._c_info(zinfo)
    out = np.zeros(data.size, dtype=np.uint8)

    def decode_all(msg):
        for _ in range(n_clouds):
            assert L.cldn_amd_decode_noheader(C.byref(ci), api._ptr(msg), msg.size, api._ptr(out), out.size) == out.size
    rows = [(tag, threads, on) for tag in bodies for threads in (1, 16) for on in (False, True)]
    times = {row: [] for row in rows}
    for r in range(WARM + REPS):
        for row in rows:
            tag, threads, on = row
            api.set_stage2_threads(threads)
            api.set_device_zstd_decode(on)
            api.set_device_zstd_sequences(on and SEQ)
            try:
                t = one(lambda: decode_all(bodies[tag]), lambda: None)
            finally:
                api.set_device_zstd_decode(False)
                api.set_device_zstd_sequences(False)
            if r >= WARM:
                times[row].append(t)
    for (tag, threads, on), t in times.items():
        print(f"decode {wl} x{n_clouds}, host messages ({tag}), {threads:2d} stage-2 thread(s), switch{'es' if SEQ else ''} {'on ' if on else 'off'}: {fmt(t)} "
              f"({np.median(t)/n_clouds*1e3:.3f} ms per message)")
