#!/usr/bin/env python3
"""applyVizLossyPreprocessing: device-resident rate of cldn_hip_viz_preprocess against the reference on one host core, then the
batch lines: cldn_hip_viz_preprocess_batch against the sum of the single-cloud calls on the same clouds, and the fused filter +
encode call (cldn_hip_encode_stage1_viz), everything device resident."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth
from cloudini_amd.schema import PointField

dev = torch.device("cuda", 0)
for n, res in ((1_000_000, 0.001), (1_000_000, 0.05), (10_000_000, 0.01)):
    info, data = synth.lidar_xyzi(n, seed=5)
    info = info.copy(fields=[PointField(f.name, f.offset, f.type, res) if i < 3 else f for i, f in enumerate(info.fields)])
    codec = native.Codec(native.Plan(info), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    d_in = torch.from_numpy(data).to(dev)
    d_out = torch.empty(data.size, dtype=torch.uint8, device=dev)
    for _ in range(2):
        kept = codec.viz_preprocess_device(d_in.data_ptr(), n, 16, 0, res, d_out.data_ptr(), data.size)
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        kept = codec.viz_preprocess_device(d_in.data_ptr(), n, 16, 0, res, d_out.data_ptr(), data.size)
    dt = (time.perf_counter() - t0) / reps
    line = f"{n} pts @ {res}: kept {kept} ({100*kept/n:.1f} %), {dt*1e3:.3f} ms per call = {n/dt/1e6:.0f} Mpoints/s"
    try:
        from oracle.binding import RefLib
        ref = RefLib()
        t0 = time.perf_counter()
        out, _, _, _ = ref.viz_preprocess(info, data)
        tr = time.perf_counter() - t0
        assert len(out) // 16 == kept
        line += f"; reference on one core {tr*1e3:.1f} ms = {n/tr/1e6:.1f} Mpoints/s"
    except (OSError, FileNotFoundError):
        pass
    print(line)
    codec.close()


def _timed(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for name, make, count, res in (("32 x 1 M XYZI", lambda k: synth.lidar_xyzi(1_000_000, seed=5 + k % 4, res=0.05), 32, 0.05),
                               ("64 x 130 k Velodyne", lambda k: synth.velodyne_xyzir(130048, seed=42 + k % 4, res=0.25), 64, 0.25)):
    distinct = [make(k) for k in range(4)]
    info = distinct[0][0]
    step = info.point_step
    data = np.concatenate([distinct[k % 4][1] for k in range(count)])
    npts = np.array([distinct[k % 4][1].size // step for k in range(count)], dtype=np.uint64)
    total = int(npts.sum())
    plan = native.Plan(info)
    codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    d_in = torch.from_numpy(data).to(dev)
    d_out = torch.empty(data.size, dtype=torch.uint8, device=dev)
    starts = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64) * step
    kept_b = codec.viz_preprocess_batch_device(d_in.data_ptr(), npts, step, 0, res, d_out.data_ptr(), data.size)

    def singles():
        return [codec.viz_preprocess_device(d_in.data_ptr() + int(starts[k]), int(npts[k]), step, 0, res,
                                            d_out.data_ptr() + int(starts[k]), int(npts[k]) * step) for k in range(count)]
    assert [int(k) for k in kept_b] == singles()
    t_batch = _timed(lambda: codec.viz_preprocess_batch_device(d_in.data_ptr(), npts, step, 0, res, d_out.data_ptr(), data.size))
    t_single = _timed(singles, reps=3)
    cap = int(sum(plan.stage1_bound(int(n)) for n in npts))
    d_enc = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(count + 1, dtype=torch.int64, device=dev)
    t_fused = _timed(lambda: codec.encode_viz_device(d_in.data_ptr(), npts, 0, res, d_enc.data_ptr(), cap, d_offs.data_ptr()))
    d_flt = torch.empty(data.size, dtype=torch.uint8, device=dev)

    def two_calls():
        kept = codec.viz_preprocess_batch_device(d_in.data_ptr(), npts, step, 0, res, d_flt.data_ptr(), data.size)
        codec.encode_device(d_flt.data_ptr(), kept, d_enc.data_ptr(), cap, d_offs.data_ptr())
    t_two = _timed(two_calls)
    print(f"batch {name} @ {res}: kept {int(kept_b.sum())} of {total} ({100 * int(kept_b.sum()) / total:.1f} %); filter alone "
          f"{t_batch * 1e3:.3f} ms = {total / t_batch / 1e6:.0f} Mpoints/s (sum of {count} single-cloud calls {t_single * 1e3:.3f} ms, "
          f"{t_single / t_batch:.2f} x); filter + encode fused {t_fused * 1e3:.3f} ms = {total / t_fused / 1e6:.0f} Mpoints/s "
          f"(batch filter, then the plain encode call: {t_two * 1e3:.3f} ms)")
    codec.close()
