"""The STRICT accept / reject rules of an LZ4 block decoder, as a small serial function (test helper).

cloudini_amd/csrc/lz4_decode.hip implements exactly these rules. They are one-sided against liblz4: wherever `decode`
accepts, LZ4_decompress_safe accepts with the same size and bytes; liblz4 additionally accepts some damaged blocks (its
shortcut paths skip end-of-block checks, and it copies whatever the destination held for a match offset of 0).

Besides the rules: the system liblz4 through ctypes, the payload kinds of tests/test_device_lz4.py, a fixed-seed corpus of
damaged blocks and an enumerated table with one block per rule line next to its accepted neighbour."""
import ctypes as C

import numpy as np

LZ4_SO = "/usr/lib/x86_64-linux-gnu/liblz4.so.1"
MFLIMIT, LASTLITERALS, MINMATCH = 12, 5, 4
REJECTED = 0xFFFFFFFF

_lz4 = None


def lz4():
    global _lz4
    if _lz4 is None:
        _lz4 = C.CDLL(LZ4_SO)
    return _lz4


def decode(block: bytes, capacity: int):
    """The decoded bytes, or None when the strict rules refuse the block."""
    b = bytes(block)
    n_in = len(b)
    if n_in == 0:
        return None
    if capacity == 0:
        return b"" if (n_in == 1 and b[0] == 0) else None
    out = bytearray()
    ip = 0
    while True:
        if ip >= n_in:
            return None
        token = b[ip]
        ip += 1
        ll = token >> 4
        if ll == 15:
            if ip >= n_in - 15:
                return None
            while True:
                s = b[ip]
                ip += 1
                ll += s
                if ip > n_in - 15:
                    return None
                if s != 255:
                    break
        if len(out) + ll > capacity - MFLIMIT or ip + ll > n_in - (2 + 1 + LASTLITERALS):  # the last sequence
            if ip + ll != n_in or len(out) + ll > capacity:
                return None
            out += b[ip:ip + ll]
            return bytes(out)
        out += b[ip:ip + ll]
        ip += ll
        offset = b[ip] | (b[ip + 1] << 8)
        ip += 2
        ml = token & 15
        if ml == 15:
            if ip >= n_in - LASTLITERALS + 1:
                return None
            while True:
                s = b[ip]
                ip += 1
                ml += s
                if ip > n_in - LASTLITERALS + 1:
                    return None
                if s != 255:
                    break
        ml += MINMATCH
        if offset == 0 or offset > len(out):  # offset 0: refused on purpose (liblz4 copies stale destination bytes)
            return None
        if len(out) + ml > capacity - LASTLITERALS:
            return None
        start = len(out) - offset
        if offset >= ml:
            out += out[start:start + ml]
        else:  # overlapping: byte-by-byte semantics = the last `offset` bytes repeated
            pattern = bytes(out[start:])
            out += (pattern * (ml // offset + 1))[:ml]


def lz4_compress(payload: bytes) -> bytes:
    cap = lz4().LZ4_compressBound(len(payload))
    out = C.create_string_buffer(max(1, cap))
    n = lz4().LZ4_compress_default(bytes(payload), out, len(payload), cap)
    assert n > 0
    return out.raw[:n]


def lz4_decompress_safe(block: bytes, capacity: int):
    """liblz4's verdict: the decoded bytes or None. 64 guard bytes behind the capacity are checked."""
    out = C.create_string_buffer(b"\xAA" * (capacity + 64), capacity + 64)
    src = C.create_string_buffer(bytes(block), max(1, len(block)))
    n = lz4().LZ4_decompress_safe(src, out, len(block), capacity)
    assert out.raw[capacity:] == b"\xAA" * 64
    return out.raw[:n] if n >= 0 else None


def payload_kinds(rs, n):
    """The payload kinds of tests/test_device_lz4.py."""
    yield "random", rs.randint(0, 256, n).astype(np.uint8).tobytes()
    yield "zeros", bytes(n)
    yield "four_symbols", rs.randint(0, 4, n).astype(np.uint8).tobytes()
    yield "period7", (bytes(range(7)) * (n // 7 + 1))[:n]
    yield "sparse_matches", bytes(b if (i // 5) % 2 else (i * 37) & 0xff for i, b in enumerate(rs.randint(0, 3, n).astype(np.uint8)))


# sizes of tests/test_device_lz4.py plus the neighbourhood of the format's reach
PAYLOAD_SIZES = list(range(0, 24)) + [63, 64, 65, 255, 256, 270, 1000, 4096, 8191, 8192, 8193, 8204, 8208, 16383, 16384, 16385,
                                      32768 + 11, 65535, 65536, 65537, 70001]


def period_65535(n: int = 140000) -> bytes:
    """Random bytes repeated with a period of 65535: liblz4 finds matches at the largest offset the format has."""
    base = np.random.RandomState(65535).randint(0, 256, 65535).astype(np.uint8).tobytes()
    return (base * (n // 65535 + 1))[:n]


def damaged(rs, block: bytes) -> bytes:
    a = bytearray(block)
    kind = rs.randint(0, 6)
    if kind == 0 and a:
        for _ in range(rs.randint(1, 4)):
            a[rs.randint(0, len(a))] = rs.randint(0, 256)
    elif kind == 1 and a:
        a = a[: rs.randint(0, len(a))]
    elif kind == 2:
        a += bytes(rs.randint(0, 256, rs.randint(1, 20)).astype(np.uint8))
    elif kind == 3 and a:
        i = rs.randint(0, len(a))
        a[i] = 0xFF if rs.randint(2) else 0xF0 | (a[i] & 15)
    elif kind == 4 and len(a) > 2:
        i = rs.randint(0, len(a) - 1)
        a[i] = 0
        a[i + 1] = 0
    return bytes(a)


def _small_payload(rs) -> bytes:
    n = int(rs.choice([0, 1, 5, 12, 13, 17, 40, 100, 300, 700]))
    k = rs.randint(0, 4)
    if k == 0:
        return rs.randint(0, 256, n).astype(np.uint8).tobytes()
    if k == 1:
        return bytes(n)
    if k == 2:
        return rs.randint(0, 3, n).astype(np.uint8).tobytes()
    return (bytes(range(7)) * (n // 7 + 1))[:n]


def _large_payload(rs) -> bytes:
    n = int(rs.randint(64 * 1024, 140 * 1024))
    k = rs.randint(0, 3)
    if k == 0:
        return rs.randint(0, 4, n).astype(np.uint8).tobytes()
    if k == 1:
        return period_65535(n)
    return bytes((i * i >> 7) & 0xff for i in range(n))


def damaged_corpus(seeds: int = 150, trials: int = 25, large_seeds: int = 6, large_trials: int = 8):
    """Fixed-seed list of (block, capacity): liblz4 blocks of small (<= 700 B) and large (64-140 KB) payloads, intact and
    damaged six ways, at capacities around the true size."""
    cases = []
    for seed in range(seeds):
        rs = np.random.RandomState(seed)
        p = _small_payload(rs)
        blk = lz4_compress(p)
        for trial in range(trials):
            b = blk if trial == 0 else damaged(rs, blk)
            for cap in (len(p), len(p) + 3, len(p) + 64, max(0, len(p) - 1), len(p) + 11, len(p) + 12):
                cases.append((b, cap))
    for seed in range(large_seeds):
        rs = np.random.RandomState(10000 + seed)
        p = _large_payload(rs)
        blk = lz4_compress(p)
        for trial in range(large_trials):
            b = blk if trial == 0 else damaged(rs, blk)
            for cap in (len(p), len(p) + 12, len(p) - 1):
                cases.append((b, cap))
    return cases


def _seq(lits: bytes, offset=None, ml=None) -> bytes:
    """One sequence; offset None = the last one (literals only). ml = the match length (>= 4)."""
    ll = len(lits)
    tok_l = min(ll, 15)
    tok_m = 0 if offset is None else min(ml - 4, 15)
    out = bytearray([(tok_l << 4) | tok_m])
    if ll >= 15:
        x = ll - 15
        while x >= 255:
            out.append(255)
            x -= 255
        out.append(x)
    out += lits
    if offset is not None:
        out += bytes([offset & 255, offset >> 8])
        if ml - 4 >= 15:
            x = ml - 4 - 15
            while x >= 255:
                out.append(255)
                x -= 255
            out.append(x)
    return bytes(out)


# 40 bytes, 68 decoded: 8 literals + match (offset 8, 8 bytes) | 3 literals + match (offset 2, 29 bytes: a length byte) |
# 20 literals (a length byte)
BASE40 = _seq(b"ABCDEFGH", 8, 8) + _seq(b"xyz", 2, 29) + _seq(bytes(range(100, 120)))
assert len(BASE40) == 40
_TAIL12 = bytes(range(200, 212))


def reject_table():
    """(name, block, capacity, accepted): one block per rule line next to its accepted neighbour."""
    t = [("base", BASE40, 68, True), ("base, room to spare", BASE40, 200, True),
         ("output one byte over capacity", BASE40, 67, False),
         ("empty input", b"", 10, False),
         ("capacity 0, block 00", b"\x00", 0, True), ("capacity 0, other block", b"\x10A", 0, False),
         ("capacity 0, two bytes", b"\x00\x00", 0, False),
         ("empty block with room", b"\x00", 64, True)]
    for n in range(40):  # (9 bytes = a token and its 8 literals: a valid last sequence, the token's match bits are not looked at)
        t.append((f"base truncated to {n}", BASE40[:n], 68, n == 9))
    for off, ok in ((0, False), (1, True), (8, True), (9, False)):  # offset 0 / offset = out + 1 and their neighbours
        t.append((f"first match at offset {off} of 8", _seq(b"ABCDEFGH", off, 8) + _seq(_TAIL12), 28, ok))
    t.append(("offset 65535 of 65535", _seq(bytes(65535), 65535, 20) + _seq(_TAIL12), 65535 + 32, True))
    # literal run one byte past the input / exact
    t.append(("last literals exact", _seq(b"ABCDEFGH", 8, 8) + b"\x50" + b"12345", 21, True))
    t.append(("last literals one past the input", _seq(b"ABCDEFGH", 8, 8) + b"\x60" + b"12345", 22, False))
    t.append(("last literals one short of the input", _seq(b"ABCDEFGH", 8, 8) + b"\x40" + b"12345", 22, False))
    # length extensions that run to the end of the input
    t.append(("literal length bytes to the end", b"\xf0" + b"\xff" * 30, 10000, False))
    t.append(("match length bytes to the end", b"\x8f" + b"ABCDEFGH" + b"\x08\x00" + b"\xff" * 20, 10000, False))
    t.append(("literal length byte inside the last 15", b"\xf0\x00" + bytes(14), 15, False))
    t.append(("literal length byte in front of the last 15", b"\xf0\x00" + bytes(15), 15, True))
    t.append(("two literal length bytes in front of the last 15", b"\xf0\xff\x00" + bytes(270), 270, True))
    # a match may not end inside the last 5 bytes of the capacity
    blk = _seq(b"ABCDEFGH", 8, 9) + _seq(_TAIL12)
    t.append(("match ends 12 before the capacity", blk, 29, True))
    t.append(("match ends inside the last 5 bytes of the capacity", blk, 21, False))
    t.append(("match ends 5 before a capacity the tail does not fit", blk, 22, False))
    # a sequence that is not the last one needs 12 bytes of room and 8 bytes of input behind its literals
    t.append(("literals of a match sequence inside the last 12 of the capacity", _seq(b"ABCDEFGH", 8, 4) + _seq(b"12345"), 17, False))
    t.append(("overlapping run fill", _seq(b"A", 1, 300) + _seq(_TAIL12), 313, True))
    t.append(("period 3 over 1000", _seq(b"abc", 3, 1000) + _seq(_TAIL12), 1015, True))
    t.append(("period 63 over 4000", _seq(bytes(range(63)), 63, 4000) + _seq(_TAIL12), 63 + 4000 + 12, True))
    t.append(("period 64 over 4000", _seq(bytes(range(64)), 64, 4000) + _seq(_TAIL12), 64 + 4000 + 12, True))
    t.append(("period 65 over 4000", _seq(bytes(range(65)), 65, 4000) + _seq(_TAIL12), 65 + 4000 + 12, True))
    return t
