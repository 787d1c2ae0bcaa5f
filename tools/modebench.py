#!/usr/bin/env python3
"""The adaptive integer mode sweep on device-resident data: one cldn_hip_sweep_modes_clouds call, against what a user could do
before it -- four cldn_hip_encode_stage1 calls with cldn_hip_codec_force_modes set to mode 0, 1, 2 and 3 for every field (which
give stream totals only, not per-field figures). Both run in the same process, alternating, 5 repetitions after one warm-up;
medians and spreads (max - min). The sweep is wanted below the loop by more than the larger of the two spreads.
`modebench.py once` runs the sweep call a few times and nothing else (for a kernel trace)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth

dev = torch.device("cuda", 0)
REPS = 5
ONCE = len(sys.argv) > 1 and sys.argv[1] == "once"


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for name, make, count in (("16 x 1 M XYZRGBA", lambda k: synth.depthcam_xyzrgba(1280, 800, seed=5 + k % 4), 16),
                          ("64 x 130 k Velodyne", lambda k: synth.velodyne_xyzir(130048, seed=42 + k % 4), 64)):
    distinct = [make(k) for k in range(4)]
    info = distinct[0][0]
    step = info.point_step
    data = np.concatenate([distinct[k % 4][1] for k in range(count)])
    npts = np.array([distinct[k % 4][1].size // step for k in range(count)], dtype=np.uint64)
    total = int(npts.sum())
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_in = torch.from_numpy(data).to(dev)
    codec = native.Codec(native.Plan(info), device=0, stream=stream)
    na = codec.plan.adaptive_fields
    d_cells = torch.zeros(count * na * 40, dtype=torch.uint8, device=dev)
    cap = int(sum(codec.plan.stage1_bound(int(n)) for n in npts))
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)

    def sweep():
        codec.sweep_modes_device(d_in.data_ptr(), npts, report_ptr=d_cells.data_ptr())

    def loop():
        for m in range(4):
            codec.force_modes([m] * na)
            codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())
        codec.force_modes(None)

    if ONCE:
        for _ in range(3):
            _once(sweep)
        rep = d_cells.cpu().numpy().view(native.MODE_DTYPE).reshape(count, na)
        print(f"{name}: {total} points, {data.size} bytes, {na} adaptive field(s); bytes per mode {rep['bytes'].sum(axis=(0, 1)).tolist()}, "
              f"probed {np.bincount(rep['probe_mode'].ravel(), minlength=4).tolist()}, best {np.bincount(rep['best_mode'].ravel(), minlength=4).tolist()}")
        codec.close()
        continue
    _once(sweep), _once(loop)  # warm-up
    t_sweep, t_loop = [], []
    for _ in range(REPS):
        t_sweep.append(_once(sweep))
        t_loop.append(_once(loop))
    ms, ml = float(np.median(t_sweep)), float(np.median(t_loop))
    ss, sl = max(t_sweep) - min(t_sweep), max(t_loop) - min(t_loop)
    print(f"{name}: mode sweep of {na} field(s): median {ms*1e3:.3f} ms per call (spread {ss*1e3:.3f} ms), "
          f"{total/ms/1e9:.2f} Gpoints/s, {data.size/ms/1e9:.1f} GB/s of {data.size/1e9:.3f} GB input")
    print(f"{name}: 4 x encode_stage1 with forced modes: median {ml*1e3:.3f} ms (spread {sl*1e3:.3f} ms); loop / sweep = {ml/ms:.2f}; "
          f"sweep below the loop by {(ml-ms)*1e3:.3f} ms, larger spread {max(ss, sl)*1e3:.3f} ms: "
          f"{'holds' if ml - ms > max(ss, sl) else 'DOES NOT HOLD'}")
    codec.close()
