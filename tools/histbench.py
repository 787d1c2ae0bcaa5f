#!/usr/bin/env python3
"""The byte histograms on device-resident data (cldn_hip_sweep_hist_*, cldn_hip_stream_hist*), in the pattern of
tools/sweepbench.py: same process, alternating, one warm-up, 5 repetitions, medians and spreads (max - min).
  k_sweep_hist   one cldn_hip_sweep_hist_clouds call, 8 rungs on every lossy float field, for several walk lengths
                 (cldn_hip_debug_hist_walk: 1024-point blocks per workgroup)
  k_stream_hist  one cldn_hip_stream_hist call over the encoded streams: bytes read per second
  three calls    what the transcoder adds behind an encode call for --estimate: sweep_hist_last_encode with the ladder, again
                 with the own resolutions, stream_hist_last_encode (device reports)
  today          what answers the same question without them: eight encode calls, each fetched to the host and compressed
                 chunk by chunk with ZSTD level 1 on 16 threads
`--kernels-only` stops behind the first two (for a counter pass)."""
import ctypes, os, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth
from cloudini_amd.build import ZSTD_SO

dev = torch.device("cuda", 0)
FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
WALKS = (1, 2, 4, 8, 16, 32)
REPS = 5
kernels_only = "--kernels-only" in sys.argv
if kernels_only:
    WALKS = (0,)  # the built-in walk only

zstd = ctypes.CDLL(ZSTD_SO)
zstd.ZSTD_compress.restype = ctypes.c_size_t
zstd.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
zstd.ZSTD_compressBound.restype = ctypes.c_size_t
zstd.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
pool = ThreadPoolExecutor(16)


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


def _zstd_chunks(stream_bytes, offs):
    """ZSTD level 1 of every chunk payload of the framed streams, on the pool; returns the compressed bytes (+ 4 per chunk)."""
    jobs = []
    for k in range(len(offs) - 1):
        at, end = int(offs[k]), int(offs[k + 1])
        while at < end:
            size = int(stream_bytes[at:at + 4].view("<u4")[0])
            jobs.append((at + 4, size))
            at += 4 + size
    base = stream_bytes.ctypes.data

    def one(job):
        cap = zstd.ZSTD_compressBound(job[1])
        dst = ctypes.create_string_buffer(cap)
        return 4 + zstd.ZSTD_compress(dst, cap, base + job[0], job[1], 1)
    return sum(pool.map(one, jobs))


for name, make, count in (("32 x 1 M XYZI", lambda k: synth.lidar_xyzi(1_000_000, seed=5 + k % 4), 32),
                          ("64 x 130 k Velodyne", lambda k: synth.velodyne_xyzir(130048, seed=42 + k % 4), 64)):
    distinct = [make(k) for k in range(4)]
    info = distinct[0][0]
    step, nf = info.point_step, len(info.fields)
    data = np.concatenate([distinct[k % 4][1] for k in range(count)])
    npts = np.array([distinct[k % 4][1].size // step for k in range(count)], dtype=np.uint64)
    total = int(npts.sum())
    lossy = [f for f, fd in enumerate(info.fields) if fd.resolution is not None and int(fd.type) in (7, 8)]
    ladders = np.zeros((nf, len(FACTORS)), dtype=np.float32)
    own = np.zeros((nf, 1), dtype=np.float32)
    for f in lossy:
        ladders[f] = [np.float32(info.fields[f].resolution * k) for k in FACTORS]
        own[f] = info.fields[f].resolution
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_in = torch.from_numpy(data).to(dev)
    codec = native.Codec(native.Plan(info), device=0, stream=stream)
    d_hist = torch.zeros(count * nf * len(FACTORS) * 2048, dtype=torch.uint8, device=dev)
    d_own = torch.zeros(count * nf * 2048, dtype=torch.uint8, device=dev)
    d_sh = torch.zeros(count * 2048, dtype=torch.uint8, device=dev)
    cap = int(sum(codec.plan.stage1_bound(int(n)) for n in npts))
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)

    # ---- k_sweep_hist per walk length
    def swept(walk):
        def run():
            codec.hist_walk(walk)
            codec.sweep_hist_clouds_device(d_in.data_ptr(), npts, ladders, report_ptr=d_hist.data_ptr())
        return run
    res = _alternate([swept(w) for w in WALKS])
    codec.hist_walk(0)
    cells = len(lossy) * len(FACTORS)
    for w, (m, s) in zip(WALKS, res):
        print(f"{name}: sweep_hist of {len(lossy)} fields x {len(FACTORS)} rungs, walk {w:2d}: median {m*1e3:.3f} ms per call (spread {s*1e3:.3f} ms), "
              f"{total/m/1e9:.2f} Gpoints/s, {total*cells/m/1e9:.1f} Gtokens/s")

    # ---- k_stream_hist over the encoded streams
    codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())
    torch.cuda.synchronize()
    offs = d_off.cpu().numpy().astype(np.uint64)
    s_bytes = int(offs[-1])
    (m, s), = _alternate([lambda: codec.stream_hist_device(d_out.data_ptr(), offs, report_ptr=d_sh.data_ptr())])
    print(f"{name}: stream_hist of {s_bytes/1e6:.1f} MB in {count} streams: median {m*1e3:.3f} ms per call (spread {s*1e3:.3f} ms), "
          f"{s_bytes/m/1e12:.3f} TB/s read")
    if kernels_only:
        codec.close()
        continue

    # ---- the transcoder's three calls behind an encode call
    codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())

    def three():
        codec.sweep_hist_last_encode(ladders, report_ptr=d_hist.data_ptr())
        codec.sweep_hist_last_encode(own, report_ptr=d_own.data_ptr())
        codec.stream_hist_last_encode(report_ptr=d_sh.data_ptr())

    def encode():
        codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())

    # ---- today: one plan and codec per rung, each stream fetched and compressed
    codecs = []
    for k in FACTORS:
        inf = info.copy()
        for f in lossy:
            inf.fields[f].resolution = float(np.float32(info.fields[f].resolution * k))
        codecs.append(native.Codec(native.Plan(inf), device=0, stream=stream))
    sizes = []
    cap2 = int(sum(codecs[0].plan.stage1_bound(int(n)) for n in npts))  # (the finest rung: the largest bound is the same for all)
    d_out2 = torch.empty(cap2, dtype=torch.uint8, device=dev)            # buffers of their own: `codec`'s last encode stays intact
    d_off2 = torch.zeros(count + 1, dtype=torch.int64, device=dev)

    def today():
        sizes.clear()
        for c in codecs:
            c.encode_device(d_in.data_ptr(), npts, d_out2.data_ptr(), cap2, d_off2.data_ptr())
            torch.cuda.synchronize()
            o = d_off2.cpu().numpy().astype(np.uint64)
            host = d_out2[:int(o[-1])].cpu().numpy()
            sizes.append(_zstd_chunks(host, o))

    (mt, st), (me, se), (ml, sl) = _alternate([three, encode, today])
    three()
    torch.cuda.synchronize()
    print(f"{name}: the three histogram calls behind an encode: median {mt*1e3:.3f} ms (spread {st*1e3:.3f} ms); the encode call itself "
          f"{me*1e3:.3f} ms (spread {se*1e3:.3f} ms)")
    print(f"{name}: {len(FACTORS)} x (encode + fetch + ZSTD-1 on 16 threads): median {ml*1e3:.1f} ms (spread {sl*1e3:.1f} ms); "
          f"today / three calls = {ml/mt:.0f}")
    # what the two say: all lossy fields moved together to each rung
    hist = d_hist.cpu().numpy().view(np.uint64).reshape(count, nf, len(FACTORS), 256).astype(np.int64)
    ownh = d_own.cpu().numpy().view(np.uint64).reshape(count, nf, 256).astype(np.int64)
    sh = d_sh.cpu().numpy().view(np.uint64).reshape(count, 256).astype(np.int64)
    for c, k in enumerate(FACTORS):
        est = sum(native.hist_entropy_bytes((sh[m_] - ownh[m_].sum(axis=0) + hist[m_, :, c].sum(axis=0)).astype(np.uint64)) for m_ in range(count))
        print(f"{name}: rung x{k:g}: estimate {est/1e6:.2f} MB, ZSTD-1 {sizes[c]/1e6:.2f} MB, estimate / actual {est/sizes[c]:.3f}")
    for c in codecs + [codec]:
        c.close()
