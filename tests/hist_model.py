"""numpy restatement of the byte histograms (include/cloudini_hip.h, cldn_hip_hist_t): no GPU, no library code.

  sweep_hist   per cloud k, field f and candidate c of the field's ladder: the 256-bin histogram of the bytes of the field's
               tokens if the field had that resolution. A token is the LEB128 varint of zig-zag(delta) + 1 -- groups of 7 bits,
               low group first, 0x80 on every byte but the last -- or the single byte 0x00 for a NaN (and for the int64 delta
               whose zig-zag + 1 wraps to 0). Quantisers, deltas and references are tests/sweep_model.py's.
  stream_hist  per stream: the histogram of all of its bytes, [u32] chunk prefixes included.
  entropy      min(N, sum over non-zero bins of c * log2(N / c) / 8), N = the sum of the bins.

A histogram ignores position: the histogram of a cloud's interleaved stream is the sum of the histograms of its parts, so
  stream_hist == sum_f sweep_hist[f][own resolution] + prefix_hist      (every field sweepable)
  stream_hist(r') - stream_hist(r) == sweep_hist[f][r'] - sweep_hist[f][r]   (field f moved from r to r')
"""
from __future__ import annotations

import numpy as np

import sweep_model as S


def token_hist(u, nan) -> np.ndarray:
    """Histogram of the varint bytes of the uint64 values u; entries with nan set, or u == 0, are the single byte 0x00."""
    u = np.where(nan, np.uint64(0), u.astype(np.uint64))
    n = np.where(u == 0, np.uint64(1), S._groups7(np.where(u == 0, np.uint64(1), u)))
    hist = np.zeros(256, dtype=np.uint64)
    for k in range(10):
        has = n > np.uint64(k)
        if not has.any():
            break
        byte = ((u >> np.uint64(7 * k)) & np.uint64(0x7F)) | np.where(n > np.uint64(k + 1), np.uint64(0x80), np.uint64(0))
        hist += np.bincount(byte[has].astype(np.int64), minlength=256).astype(np.uint64)
    return hist


def field_hist(kind, v, r) -> np.ndarray:
    """The values v of one field over one cloud (float32 or float64 array) at resolution r -> (256,) uint64."""
    r32 = np.float32(r)
    nan = np.isnan(v)
    q = S._quantise(kind, v, r32)
    ref = np.zeros(v.size, dtype=np.int64)
    ref[1:] = np.where(nan[:-1], 0, q[:-1])
    ref[::S.CHUNK] = 0
    with np.errstate(all="ignore"):
        if kind == S.FLOATN:
            d = (q.astype(np.int32).view(np.uint32) - ref.astype(np.int32).view(np.uint32)).view(np.int32)
            u = ((d.view(np.uint32) << np.uint32(1)) ^ (d >> np.int32(31)).view(np.uint32)).astype(np.uint64) + np.uint64(1)
        else:
            d = (q.view(np.uint64) - ref.view(np.uint64)).view(np.int64)
            u = ((d.view(np.uint64) << np.uint64(1)) ^ (d >> np.int64(63)).view(np.uint64)) + np.uint64(1)
    return token_hist(u, nan)


def sweep_hist(info, data, cloud_points, resolutions) -> np.ndarray:
    """data: the batch as bytes (clouds back to back). Returns the (n_clouds, n_fields, n_candidates, 256) uint64 report."""
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    res = S.check_ladders(info, resolutions)
    step = int(info.point_step)
    cloud_points = [int(n) for n in cloud_points]
    assert data.size == sum(cloud_points) * step
    kinds = S.field_kinds(info)
    rep = np.zeros((len(cloud_points), len(info.fields), res.shape[1], 256), dtype=np.uint64)
    at = 0
    for k, n in enumerate(cloud_points):
        cloud = data[at:at + n * step]
        at += n * step
        if n == 0:
            continue
        for f, (field, kind) in enumerate(zip(info.fields, kinds)):
            if kind == S.NONE:
                continue
            v = S._column(cloud, n, step, field.offset, "<f8" if kind == S.SCALAR64 else "<f4")
            for c, r in enumerate(res[f]):
                if r != 0:
                    rep[k, f, c] = field_hist(kind, v, r)
    return rep


def bytes_hist(buf) -> np.ndarray:
    return np.bincount(np.ascontiguousarray(buf).view(np.uint8).reshape(-1), minlength=256).astype(np.uint64)


def stream_hist(streams) -> np.ndarray:
    """(n_streams, 256) uint64."""
    return np.array([bytes_hist(s) for s in streams], dtype=np.uint64).reshape(len(streams), 256)


def prefix_hist(stream) -> np.ndarray:
    """Histogram of the bytes of the [u32] payload sizes of a framed stream."""
    s = np.ascontiguousarray(stream).view(np.uint8).reshape(-1)
    hist = np.zeros(256, dtype=np.uint64)
    at = 0
    while at < s.size:
        hist += bytes_hist(s[at:at + 4])
        at += 4 + int(s[at:at + 4].view("<u4")[0])
    assert at == s.size
    return hist


def entropy_bytes(hist) -> float:
    h = np.ascontiguousarray(hist, dtype=np.uint64).reshape(-1).astype(np.float64)
    n = h.sum()
    if n == 0:
        return 0.0
    c = h[h > 0]
    return float(min(n, (c * np.log2(n / c)).sum() / 8.0))


def moved(stream, own, cand) -> np.ndarray:
    """stream - own + cand, bin by bin (no bin goes below zero when `own` is part of `stream`)."""
    out = stream.astype(np.int64) - own.astype(np.int64) + cand.astype(np.int64)
    assert (out >= 0).all()
    return out.astype(np.uint64)
