"""Constructed clouds for the audit tests (test helper; nothing here calls the code under test)."""
import numpy as np

import audit_model as M
import cases
from cloudini_amd import synth
from cloudini_amd.schema import FieldType


def safe_rows(info, data):
    """Rows of a cloud inside the domain where the lossy float encoders promise anything at all: every float field that
    has a resolution is finite or NaN (NaN travels as a marker) and its tick count stays inside int32 with a margin,
    |x| / resolution < 2^31 * (1 - 2^-20). Outside it the FloatN encoder writes the 0x80000000 sentinel and +-inf has no
    tick count at all: those rows are the documented findings."""
    step = info.point_step
    n = data.size // step
    rows = np.ones(n, dtype=bool)
    for f in info.fields:
        if f.resolution is None or FieldType(f.type) not in (FieldType.FLOAT32, FieldType.FLOAT64):
            continue
        dt = "<f4" if FieldType(f.type) == FieldType.FLOAT32 else "<f8"
        size = 4 if dt == "<f4" else 8
        idx = (np.arange(n, dtype=np.int64) * step + f.offset)[:, None] + np.arange(size)[None, :]
        with np.errstate(invalid="ignore"):
            v = data[idx].copy().view(dt).reshape(-1).astype(np.float64)
        res = float(np.float32(f.resolution))
        with np.errstate(invalid="ignore"):
            rows &= np.isnan(v) | (np.abs(v) / res < 2.0 ** 31 * (1.0 - 2.0 ** -20))
    return rows


def format_bound(info, data):
    """The true per-field bound of a float32 field quantised at resolution r, from the number formats alone: half a tick of
    quantisation, plus three float32 roundings that scale with the value -- the product x * (1 / r) before rounding, the
    product ticks * r on the way back, and r and 1 / r themselves being float32 -- each at most 2^-24 relative:
        r / 2 + 3 * 2^-24 * max|x| * (1 + 2^-20).
    FLOAT64 fields: the same with 2^-53. It exceeds r as soon as |x| > r * 2^22 (2.8 km at 1 mm). Fields without a
    resolution keep 0."""
    step = info.point_step
    n = data.size // step
    lim = M.default_limits(info)
    for k, f in enumerate(info.fields):
        if f.resolution is None or FieldType(f.type) not in (FieldType.FLOAT32, FieldType.FLOAT64):
            continue
        is32 = FieldType(f.type) == FieldType.FLOAT32
        size = 4 if is32 else 8
        idx = (np.arange(n, dtype=np.int64) * step + f.offset)[:, None] + np.arange(size)[None, :]
        with np.errstate(invalid="ignore"):
            v = data[idx].copy().view("<f4" if is32 else "<f8").reshape(-1).astype(np.float64)
        v = np.abs(v[np.isfinite(v)])
        top = float(v.max()) if v.size else 0.0
        eps = 2.0 ** -24 if is32 else 2.0 ** -53
        lim[k] = max(lim[k], lim[k] / 2 + 3 * eps * top * (1 + 2.0 ** -20))
    return lim


def take_rows(data, step, rows):
    return np.ascontiguousarray(data.reshape(-1, step)[rows]).reshape(-1)


def offender_batch(seed=5, sizes=(3000, 2500, 4100)):
    """Three XYZI clouds (x y z float32 at 1 mm + uint16 intensity, 16-byte points) with one point each that a codec cannot
    carry: x = 3.0e6 m (3e9 ticks: beyond int32) at point 5 of cloud 0, y = +inf at point 7 of cloud 1."""
    info = synth.xyzi_info(sizes[0])
    clouds = []
    for k, n in enumerate(sizes):
        _, d = synth.lidar_xyzi(n, seed=seed + k)
        clouds.append(d.copy())
    clouds[0].view("<f4").reshape(-1, 4)[5, 0] = np.float32(3.0e6)
    clouds[1].view("<f4").reshape(-1, 4)[7, 1] = np.float32(np.inf)
    return info, clouds


def damage_decoded(clouds):
    """For audit_clouds only (no codec output looks like this): `a` gets a NaN in z at point 9 of cloud 1 where `b` is finite,
    `b` gets another intensity at point 11 of cloud 2. Returns (a, b) batches."""
    a = [c.copy() for c in clouds]
    b = [c.copy() for c in clouds]
    a[1].view("<f4").reshape(-1, 4)[9, 2] = np.float32(np.nan)
    b[2].view("<u2").reshape(-1, 8)[11, 6] ^= 0x0100
    return a, b


def wide_cases():
    return [(f"very_wide_{s}", *cases.very_wide_schema(s)) for s in cases.VERY_WIDE_SEEDS[::4]]
