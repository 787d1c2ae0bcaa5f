#!/usr/bin/env python3
"""Device-side LZ4 (cloudini_amd/csrc/lz4_kernels.hip): device-resident encode with stage 2 on / off, 1 and 32 clouds of
1 M XYZI points; sizes next to the system liblz4 on the same payloads.

Decode lines (cloudini_amd/csrc/lz4_decode.hip; `lz4bench.py decode` prints only these): 32 x 1 M lidar_xyzi and 16 x 1280x800
depthcam_xyzrgba, streams resident in HBM, blocks written by liblz4 (the host mirror's encoder) and by the device compressor:
decode_lz4_device against decode_device on the same clouds' stage-1 streams, the difference as GB/s of decoded payload.
Next to it the same clouds as LZ4 messages in host memory through PointcloudDecoder::decode: the host route (liblz4 on the
stage-2 pool, 1 and 16 threads) and the device route (set_device_lz4_decode). Median [min .. max] of 12 repetitions."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth

dev = torch.device("cuda", 0)


def timed(fn, sync, reps=12, warm=3):
    for _ in range(warm):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t), max(t)


def fmt(t):
    return f"{t[0]*1e3:.3f} ms [{t[1]*1e3:.3f} .. {t[2]*1e3:.3f}]"


def decode_lines():
    from cloudini_amd import api
    from cloudini_amd.schema import CompressionOption
    for wl, gen, n_clouds in (("lidar_xyzi 1M", lambda: synth.lidar_xyzi(1_000_000), 32),
                              ("depthcam_xyzrgba 1280x800", lambda: synth.depthcam_xyzrgba(1280, 800), 16)):
        info, data = gen()
        pts = data.size // info.point_step
        plan = native.Plan(info)
        codec = native.Codec(plan)
        cp = np.full(n_clouds, pts, dtype=np.uint64)
        s1 = codec.encode_host([data])[0][0]
        linfo = info.copy(compression_opt=CompressionOption.LZ4, use_threads=True)
        enc = api.PointcloudEncoder(linfo)
        body = {"liblz4": enc.encode(data)[len(enc.getHeader()):]}
        for stage2, tag in ((1, "device LZ4"), (2, "device LZ4 FAST")):
            codec.set_stage2(stage2)
            body[tag] = codec.encode_host([data])[0][0]
        codec.set_stage2(0)
        d_pts = torch.zeros(data.size * n_clouds, dtype=torch.uint8, device=dev)

        def resident(stream):
            d = torch.from_numpy(np.concatenate([stream] * n_clouds)).to(dev)
            return d, np.arange(n_clouds + 1, dtype=np.uint64) * np.uint64(stream.size)
        d_s1, o_s1 = resident(s1)
        t_s1 = timed(lambda: codec.decode_device(d_s1.data_ptr(), o_s1, cp, d_pts.data_ptr(), d_pts.numel()), codec.synchronize)
        codec.status()
        payload = (s1.size - 4 * ((pts + 32767) // 32768)) * n_clouds
        print(f"decode {wl} x{n_clouds}, HBM-resident: stage-1 streams {fmt(t_s1)} ({payload/1e6:.1f} MB of payload)")
        for tag, stream in body.items():
            d_b, o_b = resident(stream)
            t = timed(lambda: codec.decode_lz4_device(d_b.data_ptr(), o_b, cp, d_pts.data_ptr(), d_pts.numel()), codec.synchronize)
            codec.status()
            extra = t[0] - t_s1[0]
            print(f"decode {wl} x{n_clouds}, HBM-resident: LZ4 blocks by {tag} ({stream.size*n_clouds/1e6:.1f} MB) {fmt(t)} -> "
                  f"LZ4 part {extra*1e3:.3f} ms, {payload/extra/1e9:.1f} GB/s of decoded payload")
        codec.close()
        # the same clouds as LZ4 messages in host memory, one PointcloudDecoder::decode per message
        L = api.lib()
        ci, _keep = api._c_info(linfo)
        msg = np.ascontiguousarray(body["liblz4"])
        out = np.zeros(data.size, dtype=np.uint8)

        def decode_all():
            for _ in range(n_clouds):
                assert L.cldn_amd_decode_noheader(C.byref(ci), api._ptr(msg), msg.size, api._ptr(out), out.size) == out.size
        for threads in (1, 16):
            api.set_stage2_threads(threads)
            t = timed(decode_all, lambda: None)
            print(f"decode {wl} x{n_clouds}, host messages: host LZ4 route, {threads} stage-2 thread(s) {fmt(t)} "
                  f"({t[0]/n_clouds*1e3:.3f} ms per message)")
        api.set_device_lz4_decode(True)
        try:
            t = timed(decode_all, lambda: None)
        finally:
            api.set_device_lz4_decode(False)
        print(f"decode {wl} x{n_clouds}, host messages: device LZ4 route {fmt(t)} ({t[0]/n_clouds*1e3:.3f} ms per message)")


if len(sys.argv) > 1 and sys.argv[1] == "decode":
    decode_lines()
    sys.exit(0)

for wl, gen in (("c2 xyzi", lambda: synth.lidar_xyzi(1_000_000)), ("c3 depth rgba", lambda: synth.depthcam_xyzrgba(1280, 800))):
    info, data = gen()
    pts = data.size // info.point_step
    plan = native.Plan(info)
    for n_clouds in (1, 32 if wl.startswith("c2") else 16):
        codec = native.Codec(plan)
        d_in = torch.from_numpy(np.concatenate([data] * n_clouds)).to(dev)
        cp = np.full(n_clouds, pts, dtype=np.uint64)
        res = {}
        for stage2 in (0, 1, 2):
            codec.set_stage2(stage2)
            cap = plan.stage2_bound(pts, stage2) * n_clouds
            d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.zeros(n_clouds + 1, dtype=torch.int64, device=dev)
            for _ in range(3):
                codec.encode_device(d_in.data_ptr(), cp, d_out.data_ptr(), cap, d_off.data_ptr())
            codec.synchronize()
            t0 = time.perf_counter()
            reps = 10
            for _ in range(reps):
                codec.encode_device(d_in.data_ptr(), cp, d_out.data_ptr(), cap, d_off.data_ptr())
            codec.synchronize()
            codec.status()
            res[stage2] = ((time.perf_counter() - t0) / reps, int(d_off.cpu()[-1]))
        (t0_, b0) = res[0]
        for mode, tag in ((1, "device LZ4"), (2, "device LZ4 FAST")):
            (t1_, b1) = res[mode]
            print(f"{wl} x{n_clouds}: stage 1 only {t0_*1e3:.3f} ms ({b0/n_clouds/pts:.3f} B/pt); + {tag} {t1_*1e3:.3f} ms "
                  f"({b1/n_clouds/pts:.3f} B/pt, ratio {b1/b0:.4f}) -> LZ4 part {1e3*(t1_-t0_):.3f} ms, {b0/(t1_-t0_)/1e9:.1f} GB/s of payload")
        codec.close()

decode_lines()
