"""numpy restatement of the resolution sweep (include/cloudini_hip.h, cldn_hip_sweep_cell_t): no GPU, no library code.

For every cloud k, field f of the schema (in schema order) and candidate c of the field's ladder, one cell:
  bytes         bytes of the field's tokens in the cloud's regular streams if the field had this resolution
  n_class_diff  exactly one of (value, decoded value) NaN, or either +-inf and their bit patterns differ
  n_over_limit  both finite and |double(value) - double(decoded)| > double(resolution)
  max_abs_err   max of |double(value) - double(decoded)| over points with both sides finite; 0 if none

A field is sweepable when the codec encodes it with a lossy float encoder: FLOAT32 or FLOAT64 with a resolution under
EncodingOptions.LOSSY. Every other field, and every ladder entry of 0 ("skip"), gives zero cells.

Arithmetic (the reference's encoders and decoders):
  FloatN group  the 3 or 4 leading FLOAT32 fields with a resolution (src/codec_common.cpp:69-82), when their count is 3 or 4:
                m = float32(1) / r, q = int32(rint(float32(v * m))) -- half to even, 0x80000000 when NaN or out of
                [-2^31, 2^31) --, int32 wrap-around delta, zig-zag(+1) varint of 1..5 bytes
  other lossy   m = T(1.0 / float64(T(r))), q = int64(round(T(v * m))) -- half away from zero, INT64_MIN when out of range --,
                int64 wrap-around delta, zig-zag(+1) varint of 1..10 bytes (INT64_MIN's own token is the single byte 0x00)
  a NaN costs 1 byte; the reference of point i is 0 if i % 32768 == 0 or point i - 1 is a NaN, else q[i - 1]
  decoded       float32(q) * r for FLOAT32 (one float32 rounding each), float64(q) * float64(r) for FLOAT64; NaN for a NaN
"""
from __future__ import annotations

import numpy as np

from cloudini_amd.schema import EncodingOptions, FieldType

DTYPE = np.dtype([("bytes", "<u8"), ("n_class_diff", "<u8"), ("n_over_limit", "<u8"), ("max_abs_err", "<f8")])
MAX_CANDIDATES = 16
CHUNK = 32768
LADDER_FACTORS = (1.0, 0.37, 0.5, 2.5, 10.0)

NONE, FLOATN, SCALAR32, SCALAR64 = 0, 1, 2, 3


def field_kinds(info):
    """Per field: FLOATN, SCALAR32, SCALAR64, or NONE for a field that is not sweepable."""
    lossy = EncodingOptions(info.encoding_opt) == EncodingOptions.LOSSY
    lead = 0
    if lossy:
        for f in info.fields:
            if FieldType(f.type) != FieldType.FLOAT32 or f.resolution is None:
                break
            lead += 1
        if lead not in (3, 4):
            lead = 0
    kinds = []
    for i, f in enumerate(info.fields):
        t = FieldType(f.type)
        if not lossy or f.resolution is None or t not in (FieldType.FLOAT32, FieldType.FLOAT64):
            kinds.append(NONE)
        elif i < lead:
            kinds.append(FLOATN)
        else:
            kinds.append(SCALAR32 if t == FieldType.FLOAT32 else SCALAR64)
    return kinds


def default_ladders(info, factors=LADDER_FACTORS) -> np.ndarray:
    """(n_fields, len(factors)) float32: a field's own resolution times each factor, rounded to float32; 1.0 times the factors
    for fields without a resolution (their ladders are ignored)."""
    out = np.zeros((len(info.fields), len(factors)), dtype=np.float32)
    for i, f in enumerate(info.fields):
        base = np.float32(1.0 if f.resolution is None else f.resolution)
        out[i] = [np.float32(float(base) * k) for k in factors]
    return out


def _column(buf, n, step, offset, dt):
    size = np.dtype(dt).itemsize
    idx = (np.arange(n, dtype=np.int64) * step + offset)[:, None] + np.arange(size, dtype=np.int64)[None, :]
    return np.ascontiguousarray(buf[idx]).view(dt).reshape(-1)


def _round_away(t):
    """std::round: half away from zero (t - trunc(t) is exact in t's format)."""
    r = np.trunc(t)
    frac = t - r
    return r + np.where(np.abs(frac) >= 0.5, np.copysign(np.ones_like(t), t), np.zeros_like(t))


def _groups7(u):
    """Bytes of a LEB128 varint of the uint64 values u (u > 0)."""
    n = np.ones(u.shape, dtype=np.uint64)
    for k in range(1, 10):
        n += (u >= np.uint64(1 << (7 * k))).astype(np.uint64)
    return n


def _quantise(kind, v, r32):
    """q as int64 (FLOATN: an int32 value) of the entries of v; NaN entries give the out-of-range sentinel and are not used."""
    with np.errstate(all="ignore"):
        if kind == FLOATN:
            m = np.float32(1.0) / r32
            t = np.rint((v * m).astype(np.float32))
            ok = (t >= np.float32(-2147483648.0)) & (t < np.float32(2147483648.0))
            return np.where(ok, np.where(ok, t, 0).astype(np.int64), np.int64(-(1 << 31)))
        if kind == SCALAR32:
            m = np.float32(1.0 / np.float64(r32))
            t = _round_away((v * m).astype(np.float32))
            ok = (t >= np.float32(-9223372036854775808.0)) & (t < np.float32(9223372036854775808.0))
        else:
            m = np.float64(1.0) / np.float64(r32)
            t = _round_away(v * m)
            ok = (t >= -9223372036854775808.0) & (t < 9223372036854775808.0)
        return np.where(ok, np.where(ok, t, 0).astype(np.int64), np.int64(-(1 << 63)))


def field_cell(kind, v, r) -> tuple:
    """One cell: the values v of one field over one cloud (float32 or float64 array) at resolution r."""
    r32 = np.float32(r)
    n = v.size
    nan = np.isnan(v)
    q = _quantise(kind, v, r32)
    ref = np.zeros(n, dtype=np.int64)
    ref[1:] = np.where(nan[:-1], 0, q[:-1])
    ref[::CHUNK] = 0
    with np.errstate(all="ignore"):
        if kind == FLOATN:
            d = (q.astype(np.int32).view(np.uint32) - ref.astype(np.int32).view(np.uint32)).view(np.int32)
            zz = ((d.view(np.uint32) << np.uint32(1)) ^ (d >> np.int32(31)).view(np.uint32)).astype(np.uint64)
            length = _groups7(zz + np.uint64(1))
        else:
            d = (q.view(np.uint64) - ref.view(np.uint64)).view(np.int64)
            u = ((d.view(np.uint64) << np.uint64(1)) ^ (d >> np.int64(63)).view(np.uint64)) + np.uint64(1)
            length = np.where(u == 0, np.uint64(1), _groups7(np.where(u == 0, np.uint64(1), u)))
        length = np.where(nan, np.uint64(1), length)
        if kind == SCALAR64:
            dec = q.astype(np.float64) * np.float64(r32)
        else:
            dec = (q.astype(np.float32) * r32).astype(np.float32)
        dec = np.where(nan, np.array(np.nan, dtype=v.dtype), dec).astype(v.dtype)
        bits = "<u4" if v.dtype.itemsize == 4 else "<u8"
        differ = np.ascontiguousarray(v).view(bits) != np.ascontiguousarray(dec).view(bits)
        va, vb = v.astype(np.float64), dec.astype(np.float64)
        a_nan, b_nan, a_inf, b_inf = np.isnan(va), np.isnan(vb), np.isinf(va), np.isinf(vb)
        class_diff = (a_nan != b_nan) | ((a_inf | b_inf) & differ)
        finite = ~(a_nan | b_nan | a_inf | b_inf)
        err = np.abs(va - vb)
        over = finite & (err > np.float64(r32))
    return (int(length.sum()), int(class_diff.sum()), int(over.sum()), float(err[finite].max()) if finite.any() else 0.0)


def decoded(kind, v, r):
    """The values a decoder returns for v at resolution r (for tests of the model itself)."""
    r32 = np.float32(r)
    q = _quantise(kind, v, r32)
    with np.errstate(all="ignore"):
        dec = q.astype(np.float64) * np.float64(r32) if kind == SCALAR64 else (q.astype(np.float32) * r32).astype(np.float32)
    return np.where(np.isnan(v), np.array(np.nan, dtype=v.dtype), dec).astype(v.dtype)


def check_ladders(info, resolutions) -> np.ndarray:
    """The argument rules of the C ABI; returns the (n_fields, n_candidates) float32 array or raises ValueError."""
    res = np.ascontiguousarray(resolutions, dtype=np.float32)
    if res.ndim != 2 or res.shape[0] != len(info.fields) or not 1 <= res.shape[1] <= MAX_CANDIDATES:
        raise ValueError("resolutions: (n_fields, 1..16)")
    for kind, row in zip(field_kinds(info), res):
        if kind == NONE:
            continue
        for r in row:
            if r == 0:
                continue
            with np.errstate(all="ignore"):
                recip = np.float32(1.0) / r
            if not (r > 0) or np.isinf(r) or recip == 0 or np.isinf(recip):
                raise ValueError(f"resolution {r!r}")
    return res


def sweep(info, data, cloud_points, resolutions) -> np.ndarray:
    """data: the batch as bytes (clouds back to back). Returns the (n_clouds, n_fields, n_candidates) report."""
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    res = check_ladders(info, resolutions)
    step = int(info.point_step)
    cloud_points = [int(n) for n in cloud_points]
    assert data.size == sum(cloud_points) * step
    kinds = field_kinds(info)
    rep = np.zeros((len(cloud_points), len(info.fields), res.shape[1]), dtype=DTYPE)
    at = 0
    for k, n in enumerate(cloud_points):
        cloud = data[at:at + n * step]
        at += n * step
        if n == 0:
            continue
        for f, (field, kind) in enumerate(zip(info.fields, kinds)):
            if kind == NONE:
                continue
            v = _column(cloud, n, step, field.offset, "<f8" if kind == SCALAR64 else "<f4")
            for c, r in enumerate(res[f]):
                if r != 0:
                    rep[k, f, c] = field_cell(kind, v, r)
    return rep


def same(x, y) -> bool:
    """Exact equality of two reports, max_abs_err by its bits."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.view(np.uint8).tobytes() == y.view(np.uint8).tobytes()
