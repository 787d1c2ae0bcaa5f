"""What the CRC-32 tests share: the kernel's geometry, read from the one place that defines it
(cloudini_amd/csrc/stage1_launch.h: kCrcThreads, kCrcLaneBytes, kCrcWaveBytes, kCrcSegmentBytes), and span batches built
around it. k_stream_crc32 cuts a span at ADDRESSES: the first lane's slice ends at the next multiple of LANE, the first
workgroup's segment SEGMENT bytes behind the span's first 128-byte line, so every length here is placed for a given start."""
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants():
    text = open(os.path.join(ROOT, "cloudini_amd", "csrc", "stage1_launch.h")).read()
    env = {}
    for name, expr in re.findall(r"constexpr uint32_t (kCrc\w+) = ([^;]+);", text):
        env[name] = int(eval(re.sub(r"(\d+)u\b", r"\1", expr), {"__builtins__": {}}, dict(env)))
    return env


_K = _constants()
THREADS, LANE, WAVE, SEGMENT = _K["kCrcThreads"], _K["kCrcLaneBytes"], _K["kCrcWaveBytes"], _K["kCrcSegmentBytes"]
assert WAVE == 64 * LANE and SEGMENT == THREADS * LANE and LANE % 16 == 0

SMALL = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65]
STARTS = [0, 1, 16 + 7, LANE - 1]      # start address modulo LANE: 0, 1, 7 and 15 modulo 16; the last leaves lane 0 one byte
CONTENTS = ["random", "zeros", "ff", "zeros_then_01"]


def lengths_for(start: int):
    """Span lengths for a span whose first byte lies `start` bytes behind a multiple of LANE: the small ones, one below / at /
    one above a lane's slice, a wave's and a workgroup's segment both as plain lengths and as the lengths that END on those
    address cuts, two and three segments, and a remainder of one byte behind them."""
    out = list(SMALL)
    for cut in (LANE, WAVE, SEGMENT):
        out += [cut - 1, cut, cut + 1]
        if start:
            out += [cut - start - 1, cut - start, cut - start + 1]
    out += [2 * SEGMENT - start, 2 * SEGMENT - start + 1, 3 * SEGMENT - start, 3 * SEGMENT - start + 1, 2 * SEGMENT, 3 * SEGMENT + 1]
    return sorted(set(n for n in out if n >= 0))


def fill(kind: str, n: int, seed: int) -> np.ndarray:
    if kind == "random":
        return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "ff":
        return np.full(n, 0xFF, np.uint8)
    a = np.zeros(n, np.uint8)
    if n:
        a[-1] = 1
    return a


def placed_batch(start: int, kind: str):
    """One buffer (to be placed at a multiple of LANE) and its offsets: every length of lengths_for(start) as a span that
    starts `start` bytes behind a multiple of LANE, with a filler span in front of each that brings the address there.
    -> (buffer, offsets uint64 [2 n + 1], expected crc uint32 [2 n]); the tested spans are the odd ones."""
    parts, sizes = [], []
    at = 0
    for k, n in enumerate(lengths_for(start)):
        pad = (start - at) % LANE
        parts += [fill("random", pad, 1000 + k), fill(kind, n, k)]
        sizes += [pad, n]
        at += pad + n
    offs = np.zeros(len(sizes) + 1, np.uint64)
    offs[1:] = np.cumsum(sizes)
    want = np.array([zlib.crc32(p.tobytes()) for p in parts], dtype=np.uint32)
    return np.concatenate(parts), offs, want


def mixed_batch(n_spans: int = 1100, seed: int = 7):
    """Spans of mixed lengths, every third one empty, a few beyond a segment."""
    rs = np.random.RandomState(seed)
    parts = []
    for k in range(n_spans):
        if k % 3 == 1:
            n = 0
        elif k % 97 == 0:
            n = SEGMENT + int(rs.randint(0, 2 * SEGMENT))
        else:
            n = int(rs.randint(1, 3 * LANE)) if k % 2 else int(rs.randint(1, 2000))
        parts.append(fill(CONTENTS[k % 4] if k % 5 == 0 else "random", n, seed + k))
    offs = np.zeros(n_spans + 1, np.uint64)
    offs[1:] = np.cumsum([p.size for p in parts])
    want = np.array([zlib.crc32(p.tobytes()) for p in parts], dtype=np.uint32)
    return parts, np.concatenate(parts), offs, want
