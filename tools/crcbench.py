#!/usr/bin/env python3
"""CRC-32 on device-resident streams (cldn_hip_stream_crc32*), in the pattern of tools/histbench.py: same process, alternating,
one warm-up, 5 repetitions, medians and spreads (max - min).
  k_stream_crc32   one cldn_hip_stream_crc32 call over the encoded streams of 32 x 1 M XYZI clouds: bytes read per second (next
                   to it belongs tools/hbm_calib.hip's read-only figure at that size), and k_stream_hist over the same bytes
  behind an encode what cldn_hip_stream_crc32_last_encode adds to an encode call with stage 2 NONE and with the ZSTD writer
                   (device results; the call reads the offsets back once)"""
import os, sys, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth

dev = torch.device("cuda", 0)
REPS = 5


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(fns):
    for f in fns:
        _once(f)  # warm-up
    t = [[] for _ in fns]
    for _ in range(REPS):
        for k, f in enumerate(fns):
            t[k].append(_once(f))
    return [(float(np.median(x)), max(x) - min(x)) for x in t]


name, count = "32 x 1 M XYZI", 32
distinct = [synth.lidar_xyzi(1_000_000, seed=5 + k) for k in range(4)]
info = distinct[0][0]
step = info.point_step
data = np.concatenate([distinct[k % 4][1] for k in range(count)])
npts = np.array([distinct[k % 4][1].size // step for k in range(count)], dtype=np.uint64)
stream = torch.cuda.current_stream(dev).cuda_stream
d_in = torch.from_numpy(data).to(dev)
codec = native.Codec(native.Plan(info), device=0, stream=stream)
cap = int(sum(codec.plan.stage2_bound(int(n), native.STAGE2_ZSTD) for n in npts))
d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
d_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)
d_crc = torch.zeros(count, dtype=torch.int32, device=dev)
d_len = torch.zeros(count, dtype=torch.int64, device=dev)
d_sh = torch.zeros(count * 2048, dtype=torch.uint8, device=dev)

codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())
torch.cuda.synchronize()
offs = d_off.cpu().numpy().astype(np.uint64)
s_bytes = int(offs[-1])
(mc, sc), (mh, sh) = _alternate([lambda: codec.stream_crc32_device(d_out.data_ptr(), offs, crc_ptr=d_crc.data_ptr()),
                                 lambda: codec.stream_hist_device(d_out.data_ptr(), offs, report_ptr=d_sh.data_ptr())])
host = d_out[:s_bytes].cpu().numpy()
want = [zlib.crc32(host[int(a):int(b)].tobytes()) for a, b in zip(offs[:-1], offs[1:])]
assert [int(x) & 0xffffffff for x in d_crc.cpu().numpy()] == want
print(f"{name}: stream_crc32 of {s_bytes/1e6:.1f} MB in {count} streams: median {mc*1e3:.3f} ms per call (spread {sc*1e3:.3f} ms), "
      f"{s_bytes/mc/1e12:.3f} TB/s read; stream_hist of the same bytes {mh*1e3:.3f} ms (spread {sh*1e3:.3f} ms), {s_bytes/mh/1e12:.3f} TB/s")

for label, stage2 in (("stage 2 NONE", native.STAGE2_NONE), ("the ZSTD writer", native.STAGE2_ZSTD)):
    codec.set_stage2(stage2)

    def encode():
        codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())

    def encode_and_crc():
        encode()
        codec.stream_crc32_last_encode(crc_ptr=d_crc.data_ptr(), sizes_ptr=d_len.data_ptr())
    (me, se), (mb, sb) = _alternate([encode, encode_and_crc])
    assert [int(x) & 0xffffffff for x in d_crc.cpu().numpy()] == want
    print(f"{name}, {label}: encode {me*1e3:.3f} ms (spread {se*1e3:.3f} ms); encode + stream_crc32_last_encode {mb*1e3:.3f} ms "
          f"(spread {sb*1e3:.3f} ms): + {(mb-me)*1e3:.3f} ms")
codec.close()
