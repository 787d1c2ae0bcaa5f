"""Hand-built payloads for the device ZSTD writer (cloudini_amd/csrc/zstd_kernels.hip), one per block kind, header form and
threshold of it.

The tool is that of tests/lz4_payload_grid.py: INT8 / UINT8 fields are raw copies, so for a schema of K UINT8 fields with
point_step K the stage-1 payload of a chunk IS that chunk's point bytes. RAW1 puts N payload bytes in a cloud of N points
(chunks of 32 KiB), RAW4 gives 128 KiB chunks (one full block), RAW5 160 KiB (a full block and a quarter), RAW32 1 MiB (eight
blocks). A size that a step does not reach is rounded up to it.

A case is a list of clouds plus a condition on the model's trace (zstd_lit_model.frame_info(..., trace)) of every chunk, so
that a case provably is what it was built for. The trace never supplies expected bytes: those are zstd_lit_model.frame's.
Nothing here touches a GPU; tests/test_zstd_lit_model.py holds the conditions on the CPU and sends every frame through
libzstd, tests/test_gpu_zstd_encode.py runs the cases on the device.
"""
from __future__ import annotations

import numpy as np

import cases
import zstd_lit_model as M
from cloudini_amd.schema import FieldType

CHUNK_POINTS = 32768
STEPS = {"RAW1": 1, "RAW4": 4, "RAW5": 5, "RAW32": 32}
SKEWED_SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 32768, 131072, 131072 + 32, 262144]
ALIGNMENT_CASES = ["skewed_16383", "skewed_16384", "skewed_16385", "three_byte_last_block"]   # with `out` at every alignment


def schema(name: str, n_points: int = 0):
    k = STEPS[name]
    return cases.make_info([(f"b{i}", i, FieldType.UINT8, None) for i in range(k)], k, n_points)


def chunk_payloads(schema_name: str, cloud: np.ndarray):
    cb = CHUNK_POINTS * STEPS[schema_name]
    return [cloud[o:o + cb] for o in range(0, cloud.size, cb)]


def _up(n: int, k: int) -> int:
    return (n + k - 1) // k * k


def skewed(n: int, seed: int, p: float = 0.15, top: int = 40) -> np.ndarray:
    """geometric bytes: a few frequent values, a tail of rare ones"""
    return np.minimum(np.random.RandomState(seed).geometric(p, n) - 1, top).astype(np.uint8)


def distinct(n: int, k: int, seed: int, values=None) -> np.ndarray:
    """n skewed bytes of exactly k values (0 .. k - 1, or `values`), every one present"""
    rs = np.random.RandomState(seed)
    p = 0.6 if k <= 3 else max(0.02, 6.0 / k)
    d = np.minimum(rs.geometric(p, n) - 1, k - 1)
    d[rs.permutation(n)[:k]] = np.arange(k)
    return (d if values is None else np.asarray(values)[d]).astype(np.uint8)


class Case:
    def __init__(self, name, schema_name, clouds, cond):
        self.name, self.schema, self.clouds, self.cond = name, schema_name, clouds, cond
        for c in clouds:
            assert c.dtype == np.uint8 and c.size % STEPS[schema_name] == 0, (name, c.size)

    @property
    def id(self):
        return self.name


def _smallest_schema(n: int) -> str:
    for name in ("RAW1", "RAW4", "RAW5", "RAW32"):
        if n % STEPS[name] == 0 and n <= CHUNK_POINTS * STEPS[name]:
            return name
    raise AssertionError(n)


def _kinds(T):
    return [[(b["kind"], b["form"]) for b in chunk] for chunk in T]


def _expect(kinds):
    def cond(T):
        assert _kinds(T) == kinds, (_kinds(T), kinds)
    return cond


def _form_of(n: int):
    """what a compressible block of n bytes is"""
    if n < M.MIN_HUF:
        return (M.RAW, None)
    return (M.HUF, 0 if n < 256 else 1 if n < 1024 else 2 if n < 16384 else 3)


def _build():
    out = []
    H3, RAWK, RLEK = (M.HUF, 3), (M.RAW, None), (M.RLE, None)

    # ---- sizes, each as skewed bytes: both sides of every threshold (Raw below 64, one stream below 256, the three header
    # forms, one block, a 32-byte second block, two full blocks)
    for n in SKEWED_SIZES:
        name = "RAW32" if n > 131072 else _smallest_schema(n)
        blocks = [min(M.BLOCK, n - o) for o in range(0, n, M.BLOCK)]
        out.append(Case(f"skewed_{n}", name, [skewed(n, n)], _expect([[_form_of(b) for b in blocks]])))

    # ---- the step-5 schema: 26215 points = 131075 bytes, a last block of 3 bytes
    out.append(Case("three_byte_last_block", "RAW5", [skewed(26215 * 5, 5)], _expect([[H3, RAWK]])))

    # ---- the header form follows the larger of the two sizes: a payload that compresses to a few hundred bytes keeps the form
    # of its own size; one byte less and it takes the smaller form
    for n, form in ((1024, 2), (1023, 1), (16384, 3), (16383, 2)):
        def cond(T, n=n, form=form):
            b = T[0][0]
            assert (b["kind"], b["form"]) == (M.HUF, form) and b["comp"] < (1024 if n <= 1024 else 16384) // 2, b
        out.append(Case(f"compressible_{n}", "RAW1", [distinct(n, 3, n)], cond))

    # ---- all bytes equal
    out.append(Case("one_value", "RAW1", [np.full(5000, 7, np.uint8)], _expect([[RLEK]])))
    out.append(Case("one_value_64", "RAW1", [np.full(64, 200, np.uint8)], _expect([[RLEK]])))
    out.append(Case("one_value_63", "RAW1", [np.full(63, 200, np.uint8)], _expect([[RAWK]])))
    out.append(Case("full_block_then_another_run", "RAW32", [np.concatenate([np.full(131072, 7, np.uint8), np.full(4096, 9, np.uint8)])],
                    _expect([[RLEK, RLEK]])))

    # ---- two symbols: {0, 1} has one weight (direct form), {0, 255} has 254 zero weights in front of the one that counts
    def two(desc, weights):
        def cond(T):
            b = T[0][0]
            assert b["kind"] == M.HUF and b["symbols"] == 2 and b["description"] == desc and b["weights"] == weights, b
        return cond
    out.append(Case("two_symbols_0_1", "RAW1", [distinct(5000, 2, 1)], two("direct", 1)))
    out.append(Case("two_symbols_0_255", "RAW1", [distinct(5000, 2, 2, values=[0, 255])], two("fse", 255)))

    # ---- 2, 3, 128, 129 and 256 distinct symbols: an even and an odd number of weights
    for k in (3, 128, 129, 256):
        def cond(T, k=k):
            b = T[0][0]
            assert b["kind"] == M.HUF and b["symbols"] == k and b["weights"] == k - 1 and b["description"] == "fse", b
        out.append(Case(f"distinct_{k}", "RAW1", [distinct(32768, k, k)], cond))

    # ---- uniform random bytes: Raw, because the Compressed form is not smaller
    def cond_uniform(T):
        assert [b["kind"] for b in T[0]] == [M.RAW] and T[0][0]["why_raw"] == "not smaller", T[0]
    out.append(Case("uniform", "RAW4", [np.random.RandomState(9).randint(0, 256, 131072).astype(np.uint8)], cond_uniform))

    # ---- 256 symbols of about equal counts in a short block: the tree description is what does not pay
    def cond_flat(T):
        assert T[0][0]["kind"] == M.RAW, T[0]
    out.append(Case("flat_2048", "RAW1", [np.random.RandomState(10).permutation(np.resize(np.arange(256, dtype=np.uint8), 2048))], cond_flat))

    # ---- Fibonacci counts of 24 symbols in one full block: Huffman's depths reach 23, the lengths are clamped to 11
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    data = np.random.RandomState(11).permutation(np.resize(np.repeat(np.arange(24, dtype=np.uint8), fib), 131072))

    def cond_fib(T):
        b = T[0][0]
        assert (b["kind"], b["form"]) == H3 and b["clamped"] and b["max_len"] == 11 and b["symbols"] == 24, b
    out.append(Case("fibonacci_24", "RAW4", [data], cond_fib))

    # ---- four streams that compress to very different sizes
    q = 32768
    data = np.concatenate([np.zeros(q, np.uint8), skewed(q, 22), distinct(q, 200, 23), distinct(q, 3, 24)])

    def cond_streams(T):
        b = T[0][0]
        assert b["kind"] == M.HUF and max(b["streams"]) > 4 * min(b["streams"]), b
    out.append(Case("uneven_streams", "RAW4", [data], cond_streams))

    # ---- a chunk of eight blocks: Huffman, Raw and RLE mixed
    rs = np.random.RandomState(12)
    parts = [skewed(131072, 31), rs.randint(0, 256, 131072).astype(np.uint8), np.full(131072, 3, np.uint8), distinct(131072, 129, 32),
             np.full(131072, 255, np.uint8), rs.randint(0, 256, 131072).astype(np.uint8), skewed(131072, 33, 0.4), distinct(131072, 256, 34)]
    out.append(Case("eight_blocks_mixed", "RAW32", [np.concatenate(parts)], _expect([[H3, RAWK, RLEK, H3, RLEK, RAWK, H3, H3]])))

    # ---- 1100 one-chunk clouds of 13..40 bytes, 1100 blocks: a second round of 1024 in both one-workgroup scans (k_zstd_plan over
    # the chunks, k_zstd_offsets over the blocks)
    clouds = [skewed(13 + k % 28, 100 + k) for k in range(1100)]

    def cond_many(T):
        assert len(T) == 1100 > 1024 and all(len(c) == 1 and c[0]["kind"] == M.RAW for c in T)
    out.append(Case("1100_clouds", "RAW1", clouds, cond_many))

    # ---- zero-point clouds inside a batch
    clouds = [np.zeros(0, np.uint8), skewed(100, 41), np.zeros(0, np.uint8), np.zeros(0, np.uint8), skewed(300, 42), np.zeros(0, np.uint8)]
    out.append(Case("zero_point_clouds", "RAW1", clouds, _expect([[(M.HUF, 0)], [(M.HUF, 1)]])))
    return out


_grid = None
_models = {}


def grid():
    global _grid
    if _grid is None:
        _grid = _build()
    return _grid


def case(name: str) -> Case:
    return next(c for c in grid() if c.name == name)


def batches():
    """schema -> the cases that go into one encode call, in file order"""
    out = {}
    for c in grid():
        out.setdefault(c.schema, []).append(c)
    return out


def model(c: Case):
    """per cloud of the case: [(payload, the model's frame, trace of its blocks)] of its chunks (computed once and shared)"""
    if c.name not in _models:
        rows = []
        for cloud in c.clouds:
            row = []
            for p in chunk_payloads(c.schema, cloud):
                trace = []
                frame, _ = M.frame_info(p, trace)
                row.append((p, np.frombuffer(frame, np.uint8), trace))
            rows.append(row)
        _models[c.name] = rows
    return _models[c.name]


def traces(c: Case):
    """the traces of every chunk of the case, in batch order"""
    return [t for row in model(c) for _p, _f, t in row]
