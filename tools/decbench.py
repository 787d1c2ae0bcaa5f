#!/usr/bin/env python3
"""Decode timing (device resident): BASELINE configs C2-C5, single clouds S3 / S4, and T1 / T2 whose DeltaVarint sections go through
the tile walker of k_decode_tail / k_decode_sections (argument: prefix of the case name, e.g. c3)."""
import sys, os, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth

dev = torch.device("cuda", 0)
only = sys.argv[1] if len(sys.argv) > 1 else ""
# (name, cloud, clouds of the batch[, section modes the encoder is told to write: the case is about that mode's decoder])
cases = (("c5 xyz 10M", lambda: synth.lidar_xyz(10_000_000), 1), ("c2 xyzi 32x1M", lambda: synth.lidar_xyzi(1_000_000), 32),
         ("c3 xyzrgba 16x1M", lambda: synth.depthcam_xyzrgba(1280, 800), 16), ("c4 velodyne 256x130k", lambda: synth.velodyne_xyzir(130048), 256),
         ("s3 xyzrgba 1x1M", lambda: synth.depthcam_xyzrgba(1280, 800), 1), ("s4 velodyne 1x130k", lambda: synth.velodyne_xyzir(130048), 1),
         ("t1 xyz+u64 16x1M", lambda: xyz_u64(1_000_000), 16, [0]), ("t2 u64 only 16x1M", lambda: u64_walk(1_000_000), 16))


def _cloud(fields, step, cols, n):
    from cloudini_amd.schema import CompressionOption, EncodingInfo, EncodingOptions, PointField
    info = EncodingInfo(fields=[PointField(*f) for f in fields], width=n, height=1, point_step=step, encoding_opt=EncodingOptions.LOSSY,
                        compression_opt=CompressionOption.NONE, version=5, use_threads=False)
    pts = np.zeros(n, dtype=np.dtype({"names": [f[0] for f in fields], "formats": [c.dtype for c in cols], "offsets": [f[1] for f in fields],
                                      "itemsize": step}))
    for f, c in zip(fields, cols):
        pts[f[0]] = c
    return info, pts.view(np.uint8).reshape(-1)


def xyz_u64(n):
    """t1: XYZ at 1 mm and a UINT64 counter stepping by 97 -- the 8-byte field's section is left to k_decode_tail's section decoder"""
    from cloudini_amd.schema import FieldType as F
    info, data = synth.lidar_xyz(n)
    xyz = np.frombuffer(data.tobytes(), dtype=np.float32).reshape(n, -1)
    fields = [("x", 0, F.FLOAT32, 0.001), ("y", 4, F.FLOAT32, 0.001), ("z", 8, F.FLOAT32, 0.001), ("stamp", 12, F.UINT64, None)]
    return _cloud(fields, 20, [xyz[:, 0], xyz[:, 1], xyz[:, 2], np.arange(n, dtype=np.uint64) * np.uint64(97)], n)


def u64_walk(n):
    """t2: one UINT64 field, a random walk whose deltas take 3 to 5 token bytes -- DeltaVarint sections through k_decode_sections"""
    from cloudini_amd.schema import FieldType as F
    rs = np.random.RandomState(7)
    mag = np.int64(1) << rs.randint(14, 34, n).astype(np.int64)   # zigzag + 1 of +-2^k..2^(k+1), k = 14..33: 2^15 .. 2^35 -> 3..5 bytes
    d = (mag + (rs.randint(0, 1 << 30, n).astype(np.int64) % mag)) * rs.choice(np.array([-1, 1], dtype=np.int64), n)
    return _cloud([("v", 0, F.UINT64, None)], 8, [np.cumsum(d).astype(np.uint64) + np.uint64(1 << 40)], n)


for name, make, n_clouds, *forced in cases:
    if only and not name.startswith(only):
        continue
    info, data = make()
    distinct = int(os.environ.get("DECBENCH_DISTINCT", "1"))  # the cases' generators take a seed: tile several clouds
    datas = [data]
    if distinct > 1 and n_clouds > 1:
        gen = {"c2": synth.lidar_xyzi, "c4": synth.velodyne_xyzir}.get(name[:2])
        if gen is not None:
            datas = [gen(data.size // info.point_step, seed=42 + k)[1] for k in range(distinct)]
    plan = native.Plan(info)
    codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    if os.environ.get("DECBENCH_FILL_ZERO", "0") != "0":  # CLDN_HIP_FILL_ZERO: bytes no field covers may be written as 0
        codec.set_decode_fill(True)
    if os.environ.get("DECBENCH_CLOUDS") and n_clouds > 1:
        n_clouds = int(os.environ["DECBENCH_CLOUDS"])
    step = info.point_step
    n = data.size // step
    host = np.concatenate([datas[k % len(datas)] for k in range(n_clouds)])
    d_points = torch.from_numpy(host).to(dev)
    cloud_points = np.full(n_clouds, n, dtype=np.uint64)
    cap = plan.stage1_bound(n) * n_clouds
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n_clouds + 1, dtype=torch.int64, device=dev)
    n_chunks = int(sum((int(x) + 32767) // 32768 for x in cloud_points))
    d_sizes = torch.zeros(n_chunks, dtype=torch.int32, device=dev)
    d_modes = torch.zeros(max(1, n_clouds * plan.adaptive_fields), dtype=torch.uint8, device=dev)
    if forced:
        codec.force_modes(forced[0])
    codec.encode_device(d_points.data_ptr(), cloud_points, d_out.data_ptr(), cap, d_off.data_ptr(), d_sizes.data_ptr(), d_modes.data_ptr())
    sized = d_sizes.data_ptr() if os.environ.get("DECBENCH_SIZED", "1") != "0" else 0
    torch.cuda.synchronize()
    offs = d_off.cpu().numpy().astype(np.uint64)
    d_dec = torch.zeros(host.size, dtype=torch.uint8, device=dev)
    for it in range(5):
        codec.decode_device(d_out.data_ptr(), offs, cloud_points, d_dec.data_ptr(), host.size, sized)
    torch.cuda.synchronize()
    ts = []
    for blk in range(7):
        t0 = time.perf_counter()
        reps = 10
        for it in range(reps):
            codec.decode_device(d_out.data_ptr(), offs, cloud_points, d_dec.data_ptr(), host.size, sized)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / reps)
    dt = float(np.median(ts))
    codec.status()
    print(f"{name}: decode median {dt*1e3:.3f} ms (min {min(ts)*1e3:.3f}, max {max(ts)*1e3:.3f}) -> {n*n_clouds/dt/1e6:.0f} Mpoints/s, stream {int(offs[-1])/1e6:.1f} MB, stats {codec.decode_stats()}, modes {d_modes[:plan.adaptive_fields].tolist()}")
    codec.close()
