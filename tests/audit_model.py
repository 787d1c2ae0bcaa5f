"""numpy restatement of the audit report (include/cloudini_hip.h, cldn_hip_audit_field_t): no GPU, no library code.

For every cloud k and every field f of the schema, in schema order, one record:
  n_bitwise_diff   points whose field bytes differ
  n_class_diff     float fields: exactly one side NaN, or either side +-inf and the two bit patterns differ
  n_over_limit     float fields, both sides finite: |double(a) - double(b)| > limit[f]
  first_bad_point  smallest cloud-local index counted in n_class_diff or n_over_limit, or (non-float fields, and float fields
                   with limit[f] == 0) in n_bitwise_diff; 2^64 - 1 = none
  max_abs_err      max of |double(a) - double(b)| over points with both sides finite; 0 if none
Integer fields are compared as bytes; bytes no field covers are never looked at.
"""
from __future__ import annotations

import numpy as np

from cloudini_amd.schema import FieldType

DTYPE = np.dtype([("n_bitwise_diff", "<u8"), ("n_class_diff", "<u8"), ("n_over_limit", "<u8"), ("first_bad_point", "<u8"),
                  ("max_abs_err", "<f8")])
NONE = 0xFFFFFFFFFFFFFFFF

_SIZE = {FieldType.INT8: 1, FieldType.UINT8: 1, FieldType.INT16: 2, FieldType.UINT16: 2, FieldType.INT32: 4, FieldType.UINT32: 4,
         FieldType.FLOAT32: 4, FieldType.FLOAT64: 8, FieldType.INT64: 8, FieldType.UINT64: 8}
_FLOAT = {FieldType.FLOAT32: "<f4", FieldType.FLOAT64: "<f8"}


def default_limits(info) -> np.ndarray:
    """A field that has a resolution gets that resolution (as the float32 the schema carries, widened), every other field 0."""
    return np.array([0.0 if f.resolution is None else float(np.float32(f.resolution)) for f in info.fields], dtype=np.float64)


def _field_bytes(buf: np.ndarray, n: int, step: int, offset: int, size: int) -> np.ndarray:
    """(n, size) copy of one field's bytes of n consecutive points."""
    idx = (np.arange(n, dtype=np.int64) * step + offset)[:, None] + np.arange(size, dtype=np.int64)[None, :]
    return buf[idx]


def audit(info, a, b, cloud_points, limit=None) -> np.ndarray:
    """a, b: the two batches as byte arrays (clouds back to back). Returns the (n_clouds, n_fields) report."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    b = np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    step = int(info.point_step)
    limit = default_limits(info) if limit is None else np.asarray(limit, dtype=np.float64)
    assert limit.size == len(info.fields)
    cloud_points = [int(n) for n in cloud_points]
    assert a.size == b.size == sum(cloud_points) * step
    rep = np.zeros((len(cloud_points), len(info.fields)), dtype=DTYPE)
    rep["first_bad_point"] = NONE
    at = 0
    for k, n in enumerate(cloud_points):
        ca, cb = a[at:at + n * step], b[at:at + n * step]
        at += n * step
        if n == 0:
            continue
        for f, field in enumerate(info.fields):
            size = _SIZE[FieldType(field.type)]
            assert field.offset + size <= step
            xa, xb = _field_bytes(ca, n, step, field.offset, size), _field_bytes(cb, n, step, field.offset, size)
            differ = (xa != xb).any(axis=1)
            bad = differ
            r = rep[k, f]
            r["n_bitwise_diff"] = int(differ.sum())
            if FieldType(field.type) in _FLOAT:
                dt = _FLOAT[FieldType(field.type)]
                with np.errstate(invalid="ignore"):  # (widening a signalling NaN)
                    va = np.ascontiguousarray(xa).view(dt).reshape(-1).astype(np.float64)
                    vb = np.ascontiguousarray(xb).view(dt).reshape(-1).astype(np.float64)
                a_nan, b_nan, a_inf, b_inf = np.isnan(va), np.isnan(vb), np.isinf(va), np.isinf(vb)
                class_diff = (a_nan != b_nan) | ((a_inf | b_inf) & differ)
                finite = ~(a_nan | b_nan | a_inf | b_inf)
                with np.errstate(over="ignore", invalid="ignore"):
                    err = np.abs(va - vb)
                over = finite & (err > limit[f])
                r["n_class_diff"] = int(class_diff.sum())
                r["n_over_limit"] = int(over.sum())
                r["max_abs_err"] = float(err[finite].max()) if finite.any() else 0.0
                bad = class_diff | over | (differ if limit[f] == 0.0 else False)
            hits = np.flatnonzero(bad)
            if hits.size:
                r["first_bad_point"] = int(hits[0])
    return rep


def clean(info, rep) -> bool:
    """The verdict of `cloudini_batch_transcode --audit`: no class difference, nothing over its limit, integer fields intact."""
    is_float = np.array([FieldType(f.type) in _FLOAT for f in info.fields])
    return bool((rep["n_class_diff"] == 0).all() and (rep["n_over_limit"] == 0).all() and
                (rep["n_bitwise_diff"][:, ~is_float] == 0).all())


def same(x, y) -> bool:
    """Exact equality of two reports, max_abs_err by its bits."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.view(np.uint8).tobytes() == y.view(np.uint8).tobytes()
