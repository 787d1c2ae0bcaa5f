#!/usr/bin/env python3
"""The resolution sweep on device-resident data: one cldn_hip_sweep_clouds call with 8 candidates on every lossy float field,
against the same figures from the calls that existed before it -- eight plans and codecs, each doing cldn_hip_encode_stage1 +
cldn_hip_audit_last_encode. Both run in the same process, alternating, 5 repetitions after one warm-up; medians and spreads
(max - min). The sweep is wanted below the loop by more than the larger of the two spreads."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth

dev = torch.device("cuda", 0)
FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
REPS = 5


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


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
    for f in lossy:
        ladders[f] = [np.float32(info.fields[f].resolution * k) for k in FACTORS]
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_in = torch.from_numpy(data).to(dev)
    sweeper = native.Codec(native.Plan(info), device=0, stream=stream)
    d_cells = torch.zeros(count * nf * len(FACTORS) * 32, dtype=torch.uint8, device=dev)
    # the loop of the calls that were there before: one plan and codec per candidate
    codecs = []
    for k in FACTORS:
        inf = info.copy()
        for f in lossy:
            inf.fields[f].resolution = float(np.float32(info.fields[f].resolution * k))
        codecs.append(native.Codec(native.Plan(inf), device=0, stream=stream))
    cap = int(sum(codecs[0].plan.stage1_bound(int(n)) for n in npts))
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)
    d_rep = torch.zeros(count * nf * 40, dtype=torch.uint8, device=dev)

    def sweep():
        sweeper.sweep_clouds_device(d_in.data_ptr(), npts, ladders, report_ptr=d_cells.data_ptr())

    def loop():
        for c in codecs:
            c.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())
            c.audit_last_encode(report_ptr=d_rep.data_ptr())

    _once(sweep), _once(loop)  # warm-up
    t_sweep, t_loop = [], []
    for _ in range(REPS):
        t_sweep.append(_once(sweep))
        t_loop.append(_once(loop))
    ms, ml = float(np.median(t_sweep)), float(np.median(t_loop))
    ss, sl = max(t_sweep) - min(t_sweep), max(t_loop) - min(t_loop)
    cells = len(lossy) * len(FACTORS)
    print(f"{name}: sweep of {len(lossy)} fields x {len(FACTORS)} candidates: median {ms*1e3:.3f} ms per call (spread {ss*1e3:.3f} ms), "
          f"{total/ms/1e9:.2f} Gpoints/s, {total*cells/ms/1e9:.1f} Gcells/s, {data.size/ms/1e9:.1f} GB/s of {data.size/1e9:.3f} GB input")
    print(f"{name}: {len(FACTORS)} x (encode_stage1 + audit_last_encode): median {ml*1e3:.3f} ms (spread {sl*1e3:.3f} ms); "
          f"loop / sweep = {ml/ms:.2f}; sweep below the loop by {(ml-ms)*1e3:.3f} ms, larger spread {max(ss, sl)*1e3:.3f} ms: "
          f"{'holds' if ml - ms > max(ss, sl) else 'DOES NOT HOLD'}")
    for c in codecs + [sweeper]:
        c.close()
