"""LZ4 message bodies for the tests of cldn_hip_decode_lz4 (test helper): the body of a cloud's LZ4 message built from the
oracle's stage-1 stream, a composite model of the decode (chunk chain + strict block rules + the oracle's stage-1 decoder),
the clouds the route is tested with and the ways their bodies are damaged.

Nothing here calls the code under test. `body_of` and `model` are pinned against the compiled reference on the CPU
(tests/test_decode_lz4_routes.py): the body is byte-identical to the reference's, and wherever the model accepts, the
reference accepts with the same points."""
import os

import numpy as np

import cases
import lz4_block_rules as R
from cloudini_amd.schema import CompressionOption

POINTS_PER_CHUNK = 32768


def chunks_of(stream):
    """The payloads of a well-formed [u32 size][payload] chain."""
    s = np.ascontiguousarray(stream, dtype=np.uint8)
    out, pos = [], 0
    while pos < s.size:
        size = int.from_bytes(s[pos:pos + 4].tobytes(), "little")
        out.append(s[pos + 4:pos + 4 + size])
        pos += 4 + size
    assert pos == s.size
    return out


def frame(payloads) -> np.ndarray:
    parts = []
    for p in payloads:
        p = np.frombuffer(bytes(p), dtype=np.uint8) if isinstance(p, (bytes, bytearray)) else np.asarray(p, dtype=np.uint8)
        parts.append(np.frombuffer(int(p.size).to_bytes(4, "little"), dtype=np.uint8))
        parts.append(p)
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def body_of(stage1_stream) -> np.ndarray:
    """The body of the LZ4 message of a cloud whose stage-1 stream this is: [u32 len][LZ4 block of the payload] per chunk."""
    return frame([R.lz4_compress(c.tobytes()) for c in chunks_of(stage1_stream)])


def lz4_info(info):
    return info.copy(compression_opt=CompressionOption.LZ4)


def capacity_of(oracle, info) -> int:
    """What a chunk's block may decode to: the bound of a full chunk's stage-1 payload + 60 (PointcloudDecoder::decode)."""
    return oracle.stage1_bound(info, POINTS_PER_CHUNK) + 60


def walk(body, n):
    """The chunk chain the way k_walk_chunks (stage1_decode.h) follows it: the blocks, or None for a chain that is refused."""
    b = bytes(np.ascontiguousarray(body, dtype=np.uint8).tobytes())
    pos, end, remaining, blocks = 0, len(b), int(n), []
    while pos < end:
        if remaining == 0:            # more chunks than declared points
            return None
        if end - pos < 4:             # a cut prefix
            return None
        size = int.from_bytes(b[pos:pos + 4], "little")
        pos += 4
        if size > end - pos:          # a size past the end
            return None
        blocks.append(b[pos:pos + size])
        pos += size
        remaining -= min(remaining, POINTS_PER_CHUNK)
    if remaining:                     # the data ends before all declared points
        return None
    return blocks


def refused_block(body, n, capacity) -> bool:
    """True when the chain parses and the strict rules refuse one of its blocks: the case reported as an LZ4 failure."""
    blocks = walk(body, n)
    return blocks is not None and any(R.decode(blk, capacity) is None for blk in blocks)


def payloads_of(body, n, capacity):
    """The stage-1 payloads the body's blocks decode to by the strict rules, or None (chain or a block refused)."""
    blocks = walk(body, n)
    if blocks is None:
        return None
    payloads = []
    for blk in blocks:
        p = R.decode(blk, capacity)
        if p is None:
            return None
        payloads.append(p)
    return payloads


def reference_buffer_too_small(info, body, n, capacity) -> bool:
    """The reference decompresses every chunk into width * height * point_step bytes (PointcloudDecoder::decodeChunk,
    max_decompressed_size), the library into the bound of a full chunk + 60. Where a chunk's stage-1 payload is LARGER than the
    whole cloud's points -- small clouds of full-range 64-bit integers, whose varints take 10 bytes for 8 --, the reference
    refuses the message its own encoder wrote, and the library, the host mirror with liblz4 and the model decode it. The
    CPU pins assert that refusal instead of equal points for exactly these bodies."""
    payloads = payloads_of(body, n, capacity)
    return payloads is not None and any(len(p) > int(n) * info.point_step for p in payloads)


def model(oracle, info, body, n, capacity, fill):
    """The points of the LZ4 body, or None where the decode must report corrupt data."""
    payloads = payloads_of(body, n, capacity)
    if payloads is None:
        return None
    try:
        return oracle.decode_stage1(info, frame(payloads), n, fill=fill)
    except Exception:
        return None


# ---- the clouds ---------------------------------------------------------------------------------------------------------
# Seed ranges of the schema generators of tests/test_gpu_fuzz.py that no other test uses (in use there: 1000-1100, 2000+7000..,
# 3000-3080, 5000-5040, 7000-7200, 9000-9200, 11000-11100). CLDN_FUZZ_EXTRA / CLDN_FUZZ_BASE extend them as in that file.
_EXTRA = int(os.environ.get("CLDN_FUZZ_EXTRA", "0"))
_BASE = int(os.environ.get("CLDN_FUZZ_BASE", "0"))
RANDOM_SEEDS = list(range(21000, 21100)) + list(range((_BASE or 21100) + 21_000_000, (_BASE or 21100) + 21_000_000 + _EXTRA // 10))
CORNER_SEEDS = list(range(27000, 27100)) + list(range((_BASE or 27100) + 27_000_000, (_BASE or 27100) + 27_000_000 + _EXTRA // 10))
WIDE_SEEDS = cases.VERY_WIDE_SEEDS[::4]

_families = None


def family_names():
    return [name for name, _i, _d in _family_list()]


def _family_list():
    global _families
    if _families is None:
        _families = cases.encode_cases()
    return _families


def cloud_ids():
    """Every cloud of the LZ4 decode tests as (kind, key): all schema families, very wide schemas, fresh fuzz seeds."""
    return ([("family", name) for name in family_names()] + [("wide", s) for s in WIDE_SEEDS] +
            [("random", s) for s in RANDOM_SEEDS] + [("corner", s) for s in CORNER_SEEDS])


def cloud(kind, key):
    """(info, data, number): `number` picks the legs a cloud takes and seeds its damage."""
    if kind == "family":
        names = family_names()
        _n, info, data = _family_list()[names.index(key)]
        return info, np.ascontiguousarray(data).view(np.uint8).reshape(-1), names.index(key)
    if kind == "wide":
        info, data = cases.very_wide_schema(key)
        return info, data, int(key)
    import test_gpu_fuzz as fz
    info, data = fz._random_case(key) if kind == "random" else fz._corner_case(key)
    return info, data, int(key)


# ---- damage -------------------------------------------------------------------------------------------------------------
DAMAGE_KINDS = ("body", "body2", "payload", "prefix")


def damage(kind, seed, stage1_stream, body):
    """One damaged LZ4 body. body / body2: the body's bytes, with _damage of tests/test_gpu_fuzz.py (two draws); payload: one
    chunk's stage-1 payload damaged, then compressed again (a valid block around a corrupt chunk); prefix: one [u32] replaced."""
    import test_gpu_fuzz as fz
    rs = np.random.RandomState((seed * 4 + DAMAGE_KINDS.index(kind)) & 0x7fffffff)
    if kind in ("body", "body2"):
        return fz._damage(rs, np.ascontiguousarray(body, dtype=np.uint8))
    chunks = chunks_of(stage1_stream)
    k = int(rs.randint(0, len(chunks)))
    if kind == "payload":
        p = chunks[k].copy()
        how = rs.randint(0, 4)
        if how == 0 and p.size:
            p[rs.randint(0, p.size)] ^= np.uint8(1 << rs.randint(0, 8))
        elif how == 1 and p.size:
            p = p[: rs.randint(0, p.size)]
        elif how == 2:
            p = np.concatenate([p, rs.randint(0, 256, int(rs.randint(1, 4))).astype(np.uint8)])
        elif p.size:                                 # the chunk's tail: its sections
            p[p.size - 1 - int(rs.randint(0, min(64, p.size)))] = np.uint8(rs.randint(0, 256))
        blocks = [R.lz4_compress(c.tobytes()) for c in chunks]
        blocks[k] = R.lz4_compress(p.tobytes())
        return frame(blocks)
    blocks = chunks_of(body)
    pos = sum(4 + b.size for b in blocks[:k])
    size = blocks[k].size
    new = int(rs.choice([0, 1, max(0, size - 1), size + 1, size + 4, body.size, 0xFFFFFFFF, int(rs.randint(0, 1 << 16))]))
    out = np.ascontiguousarray(body, dtype=np.uint8).copy()
    out[pos:pos + 4] = np.frombuffer(new.to_bytes(4, "little"), dtype=np.uint8)
    return out
