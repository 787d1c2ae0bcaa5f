#!/usr/bin/env python3
"""The audit on device-resident data: cldn_hip_audit_clouds on a batch and its decode (the kernel's rate), cldn_hip_audit_last_encode
as a share of the encode call it follows. With `--once`: one encode + one audit_last_encode (for a copy trace)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cloudini_amd import native, synth

dev = torch.device("cuda", 0)
once = "--once" in sys.argv


def _timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for name, make, count in (("32 x 1 M XYZI", lambda k: synth.lidar_xyzi(1_000_000, seed=5 + k % 4), 32),
                          ("64 x 130 k Velodyne", lambda k: synth.velodyne_xyzir(130048, seed=42 + k % 4), 64)):
    distinct = [make(k) for k in range(4)]
    info = distinct[0][0]
    step = info.point_step
    data = np.concatenate([distinct[k % 4][1] for k in range(count)])
    npts = np.array([distinct[k % 4][1].size // step for k in range(count)], dtype=np.uint64)
    total = int(npts.sum())
    plan = native.Plan(info)
    codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    cap = int(sum(plan.stage1_bound(int(n)) for n in npts))
    d_in = torch.from_numpy(data).to(dev)
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)
    d_dec = torch.zeros(data.size, dtype=torch.uint8, device=dev)
    d_rep = torch.zeros(count * len(info.fields) * 40, dtype=torch.uint8, device=dev)
    encode = lambda: codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr())
    encode()
    if once:
        codec.audit_last_encode(report_ptr=d_rep.data_ptr())
        torch.cuda.synchronize()
        print(f"{name}: one encode_device + one audit_last_encode (device report)")
        break
    torch.cuda.synchronize()
    offs = d_off.cpu().numpy().astype(np.uint64)
    codec.decode_device(d_out.data_ptr(), offs, npts, d_dec.data_ptr(), data.size)
    codec.status()
    rep = codec.audit_clouds_device(d_in.data_ptr(), d_dec.data_ptr(), npts)
    worst = float(rep["max_abs_err"].max())
    t_audit = _timed(lambda: codec.audit_clouds_device(d_in.data_ptr(), d_dec.data_ptr(), npts, report_ptr=d_rep.data_ptr()))
    gb = 2.0 * data.size / 1e9
    print(f"{name}: audit_clouds (device report) {t_audit*1e3:.3f} ms per call = {gb/t_audit/1e3:.2f} TB/s of {gb:.3f} GB read, "
          f"{total/t_audit/1e9:.1f} Gpoints/s; max_abs_err {worst:.6g}, findings {int(rep['n_over_limit'].sum() + rep['n_class_diff'].sum())}")
    t_enc = _timed(encode)

    def both():
        encode()
        codec.audit_last_encode(report_ptr=d_rep.data_ptr())
    t_both = _timed(both)
    t_host = _timed(lambda: (encode(), codec.audit_last_encode()))
    print(f"{name}: encode_device {t_enc*1e3:.3f} ms; + audit_last_encode (device report) {t_both*1e3:.3f} ms "
          f"(+{(t_both-t_enc)*1e3:.3f} ms = {t_both/t_enc:.2f} x the encode call); host report {t_host*1e3:.3f} ms")
    codec.close()
