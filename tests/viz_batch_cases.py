"""Ragged batches for the batched viz pre-filter (cldn_hip_viz_preprocess_batch): GPU-free, shared by the CPU test (oracle
against the compiled reference, cloud by cloud) and the GPU tests (HIP against the oracle) of tests/test_viz_batch.py.

One (point step, triple offset, resolution) per seed, from the choices of test_viz_preprocess._viz_random; 5-12 clouds of
the sizes below, with its cluster kinds. Every batch holds an all-NaN cloud, a cloud without duplicates or NaNs, a zero-point
cloud and THE SAME CLOUD TWICE IN A ROW -- two copies of a cloud with many points per voxel: a table shared between the
clouds of a batch would drop the whole second copy."""
import os

import numpy as np

import cases
from cloudini_amd.schema import FieldType as F

SIZES = [0, 1, 63, 1023, 1024, 1025, 20_000, 70_001]
_EXTRA = int(os.environ.get("CLDN_FUZZ_EXTRA", "0"))
SEEDS = list(range(31_000, 31_040)) + list(range(31_000_000, 31_000_000 + _EXTRA // 50))


def _xyz(rs, n, kind, res):
    """The cluster kinds of _viz_random."""
    if kind == 0:
        xyz = rs.uniform(-50, 50, (n, 3))
    elif kind == 1:                                              # a few hundred clusters, tight
        c = rs.uniform(-20, 20, (max(1, n // 200), 3))
        xyz = c[rs.randint(0, len(c), n)] + rs.normal(0, res * 0.7, (n, 3))
    elif kind == 2:                                              # a scan line: neighbours share voxels
        t = np.arange(n) * 1e-3
        xyz = np.stack([np.cos(t) * 10, np.sin(t) * 10, t * 0.01], axis=1)
    else:                                                        # a grid hit many times
        xyz = np.round(rs.uniform(-3, 3, (n, 3)) / (res * 2)) * (res * 2)
    return xyz.astype(np.float32)


def viz_batch(seed):
    """(info, [cloud bytes], xyz_offset, resolution, index of the first cloud of the identical pair)"""
    rs = np.random.RandomState(seed)
    off = int(rs.choice([0, 0, 1, 2, 4, 7]))
    extra = int(rs.choice([0, 0, 2, 4, 6, 20]))
    step = off + 12 + extra
    res = float(rs.choice([0.001, 0.01, 0.05, 0.25, 1.0]))
    fields = [("x", off, F.FLOAT32, res), ("y", off + 4, F.FLOAT32, res), ("z", off + 8, F.FLOAT32, res)]
    if extra >= 2:
        fields.append(("i", off + 12, F.UINT16, None))

    def pack(xyz):
        n = len(xyz)
        cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]}
        if extra >= 2:
            cols["i"] = rs.randint(0, 65536, n).astype(np.uint16)
        return cases.pack(cases.make_info(fields, step, n), cols, n)

    big = [s for s in SIZES if s >= 1023]
    n_nan = int(rs.choice([s for s in SIZES if s]))
    all_nan = pack(np.full((n_nan, 3), np.nan, dtype=np.float32))
    n_clean = int(rs.choice([s for s in SIZES if s]))
    i = np.arange(n_clean)                                       # one point per voxel, four voxels apart, all finite
    clean = pack((np.stack([i % 1000, i // 1000, np.zeros(n_clean)], axis=1) * (4 * res)).astype(np.float32))
    zero = np.zeros(0, np.uint8)
    twin = pack(_xyz(rs, int(rs.choice(big)), 1, res))           # tight clusters, no NaN: loses points to the dedup only
    units = [[all_nan], [clean], [zero], [twin, twin.copy()]]
    for _ in range(int(rs.randint(0, 8))):                       # 5-12 clouds
        n = int(rs.choice(SIZES))
        xyz = _xyz(rs, n, int(rs.randint(0, 4)), res)
        k = max(1, n // 100)
        if n and rs.rand() < 0.6:
            xyz[rs.randint(0, n, k), rs.randint(0, 3, k)] = np.nan
        if n and rs.rand() < 0.3:
            xyz[rs.randint(0, n, k), rs.randint(0, 3, k)] = rs.choice([np.inf, -np.inf, 3e9, -3e9, 2.5e6, 1e19], k).astype(np.float32)
        units.append([pack(xyz)])
    order = rs.permutation(len(units))
    clouds, twin_at = [], -1
    for u in order:
        if u == 3:
            twin_at = len(clouds)
        clouds += units[u]
    info = cases.make_info(fields, step, 0)
    return info, clouds, off, res, twin_at


def expected(oracle, seed):
    """The oracle's survivors per cloud, after the conditions every batch has to meet (checked on the CPU, on the oracle's
    counts): a cloud that loses points to the dedup alone, one that loses everything, one that loses nothing, and the
    identical pair keeping twice what one copy keeps."""
    info, clouds, off, res, twin_at = viz_batch(seed)
    step = info.point_step
    want = [oracle.viz_preprocess(c, step, off, res) for c in clouds]
    n = [c.size // step for c in clouds]
    kept = [w.size // step for w in want]
    assert 5 <= len(clouds) <= 12 and 0 in n
    assert np.array_equal(clouds[twin_at], clouds[twin_at + 1]) and kept[twin_at] == kept[twin_at + 1]
    assert 0 < kept[twin_at] < n[twin_at], seed                  # no NaN in it: the dedup alone
    assert any(k == 0 and m > 0 for k, m in zip(kept, n)), seed
    assert any(k == m and m > 0 for k, m in zip(kept, n)), seed
    return info, clouds, off, res, twin_at, want
