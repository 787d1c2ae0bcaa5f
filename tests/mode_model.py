"""numpy restatement of the adaptive integer mode sweep (include/cloudini_hip.h, cldn_hip_mode_cell_t): no GPU, no library code.

For every cloud k and adaptive field a (the V5 integer fields, schema order) one cell: the exact section bytes under each of the
four modes summed over the cloud's chunks of <= 32768 values, the mode the reference's probe commits (the selection rule on
the first min(n, 4096) values as ONE section) and the mode the same rule picks on the sums. Per section (src/v5_codec.cpp:258-316,
381-402), nothing crossing its edges:
  0 DeltaVarint  1 + sum varint64len(v[i] - v[i-1])                       int64 wrap-around, v[-1] = 0
  1 Palette      3 + U * bpv + ceil(bits(U) * n / 8)                      U distinct values, bits = bitsForPaletteIndex
  2 Rle          5 + sum over runs of equal values (bpv + uvarintlen(len))
  3 DeltaRle     5 + sum over runs of equal deltas (varint64len(delta) + uvarintlen(len))
"""
from __future__ import annotations

import numpy as np

from cloudini_amd.schema import EncodingOptions, FieldType

DTYPE = np.dtype([("bytes", "<u8", (4,)), ("probe_mode", "<u4"), ("best_mode", "<u4")])
CHUNK, PROBE = 32768, 4096
_NP = {FieldType.INT16: "<i2", FieldType.UINT16: "<u2", FieldType.INT32: "<i4", FieldType.UINT32: "<u4",
       FieldType.INT64: "<i8", FieldType.UINT64: "<u8"}


def adaptive_fields(info):
    """The fields that get a V5 section, in the order of the encode calls' `modes` (UsesV5Codec, src/v5_codec.cpp:883-892)."""
    if int(info.version) < 5 or EncodingOptions(info.encoding_opt) != EncodingOptions.LOSSY:
        return []
    return [f for f in info.fields if FieldType(f.type) in _NP]


def column(info, data, f):
    """The field's values as int64 (ToInt64<T>; UINT64 reinterpreted) and its size in bytes."""
    dt = np.dtype(_NP[FieldType(f.type)])
    pts = np.ascontiguousarray(data).view(np.uint8).reshape(-1, info.point_step)
    return pts[:, f.offset:f.offset + dt.itemsize].copy().view(dt).reshape(-1).astype(np.int64), dt.itemsize


def _varint64_len(d):
    """encodeVarint64: zig-zag + 1; INT64_MIN wraps to 0 and is one byte."""
    d = d.astype(np.int64)
    u = ((d.view(np.uint64) << np.uint64(1)) ^ (d >> np.int64(63)).view(np.uint64)) + np.uint64(1)
    out = np.ones(u.shape, dtype=np.int64)
    for k in range(1, 10):
        out += u >= np.uint64(1 << (7 * k))
    return out


def _uvarint_len(v):
    return 1 + (v >= 128) + (v >= 16384)  # run lengths are <= 32768


def _run_lengths(starts):
    idx = np.flatnonzero(starts)
    return np.diff(np.append(idx, starts.size))


def section_sizes(v, bpv):
    """The four sizes of one section of int64 values v (1..32768 of them)."""
    n = v.size
    d = v - np.concatenate([[0], v[:-1]]).astype(np.int64)  # wraps
    dl = _varint64_len(d)
    rs = np.ones(n, dtype=bool)
    rs[1:] = v[1:] != v[:-1]
    ds = np.ones(n, dtype=bool)
    ds[1:] = d[1:] != d[:-1]
    u = np.unique(v).size
    bits = 0 if u <= 1 else int(u - 1).bit_length()
    return [1 + int(dl.sum()), 3 + u * bpv + (bits * n + 7) // 8,
            5 + int(rs.sum()) * bpv + int(_uvarint_len(_run_lengths(rs)).sum()),
            5 + int(dl[ds].sum()) + int(_uvarint_len(_run_lengths(ds)).sum())]


def select(sizes):
    """selectBestAdaptiveIntMode: DeltaVarint, Palette, Rle, DeltaRle in this order, strict <."""
    best, size = 0, sizes[0]
    for m in (1, 2, 3):
        if sizes[m] < size:
            best, size = m, sizes[m]
    return best


def sweep(info, data, cloud_points) -> np.ndarray:
    """(n_clouds, adaptive fields) cells for clouds lying back to back in `data`."""
    fields = adaptive_fields(info)
    rep = np.zeros((len(cloud_points), len(fields)), dtype=DTYPE)
    first = 0
    for k, n in enumerate(cloud_points):
        cloud = np.ascontiguousarray(data).view(np.uint8)[first * info.point_step:(first + n) * info.point_step]
        first += n
        for a, f in enumerate(fields if n else []):
            v, bpv = column(info, cloud, f)
            total = np.sum([section_sizes(v[c:c + CHUNK], bpv) for c in range(0, n, CHUNK)], axis=0)
            rep[k, a] = (total, select(section_sizes(v[:PROBE], bpv)), select([int(x) for x in total]))
    return rep
