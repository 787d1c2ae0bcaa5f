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


# ---- the structural grid ------------------------------------------------------------------------------------------------
# Blocks no compressor writes: sequences placed at the constants and branches of cloudini_amd/csrc/lz4_decode.hip (lzd_block).
# The builder appends every sequence's bytes to its own payload, so the expected output depends on no decoder.

_POOL = np.random.RandomState(20240).randint(0, 256, 300000).astype(np.uint8).tobytes()   # literal bytes (never periodic)


class _Builder:
    def __init__(self):
        self.blk = bytearray()
        self.out = bytearray()

    def lits(self, n: int) -> bytes:
        """n literal bytes; which ones depends on where the output stands, so that equal runs differ between blocks."""
        at = (len(self.out) * 7 + len(self.blk)) % 30011
        return _POOL[at:at + n]

    def seq(self, ll: int, offset: int, ml: int):
        """ll literals, then ml bytes from `offset` back (byte-by-byte semantics)."""
        lit = self.lits(ll)
        self.blk += _seq(lit, offset, ml)
        self.out += lit
        assert 1 <= offset <= len(self.out) and offset <= 65535 and ml >= 4
        start = len(self.out) - offset
        if offset >= ml:
            self.out += self.out[start:start + ml]
        else:
            pattern = bytes(self.out[start:])
            self.out += (pattern * (ml // offset + 1))[:ml]
        return self

    def fast_chain(self, n_bytes: int):
        """Exactly n_bytes (0 or >= 3) of input made of sequences the fast path takes: no length bytes, 3..17 bytes each."""
        assert n_bytes == 0 or n_bytes >= 3
        k = 0
        while n_bytes:
            s = min(n_bytes, 17 if k % 2 else 11)
            if 0 < n_bytes - s < 3:
                s = n_bytes - 3
            ll = s - 3
            have = len(self.out) + ll
            self.seq(ll, 1 + (k * 5) % min(have, 40), 4 + k % 15)
            n_bytes -= s
            k += 1
        return self

    def short_chain(self, n_bytes: int):
        """n_bytes (>= 0) of input made of sequences with literal runs of 15..269 bytes (window copies, one length byte each):
        what is left below a sequence's smallest size goes into fast-path sequences."""
        while n_bytes >= 5 + 15 + 3:
            ll = min(n_bytes - 5 - 3, 15 + (len(self.blk) * 13) % 240)      # 1 token + 1 length byte + ll + 2 offset + 1 match byte
            if 0 < n_bytes - (5 + ll) < 3:
                ll += n_bytes - (5 + ll)                                    # (ll stays below 270: one length byte)
            self.seq(ll, 1 + len(self.blk) % 60, 19 + len(self.blk) % 200)
            n_bytes -= 5 + ll
        return self.fast_chain(n_bytes)

    def end(self, tail: int = 12):
        lit = self.lits(tail)
        self.blk += _seq(lit)
        self.out += lit
        return bytes(self.blk), bytes(self.out)


def _lead_in(style: str, p: int) -> "_Builder":
    """A block whose next sequence starts p input bytes behind the point where the decoder last re-based its look-ahead
    (style fast: lzd_block loads the look-ahead at the offset bytes of a general-path sequence, 2 bytes in front of the
    chain), behind one literal run of p bytes (lit) or behind p bytes of window-copied literal runs (short)."""
    b = _Builder()
    if style == "lit":
        return b.seq(max(p, 1), 1, 19)          # (ml 19: a length byte, so that the sequence takes the general path for every p)
    b.seq(6, 3, 19)
    return b.fast_chain(p) if style == "fast" else b.short_chain(p)


_FIXED = {"a": (3, 6), "b": (20, 30), "c": (15 + 255 + 2, 4 + 15 + 255 + 7)}   # (literals, match length): 0 / 1 / 2 length bytes each
_LIT_RUNS = [14, 15, 16, 63, 64, 65, 269, 270, 271, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385,
             32767, 32768, 32769, 65535, 65536, 65537]
_LONG_ML = [63, 64, 65, 16383, 16384, 16385, 40000, 70000]
_WRAP_D = [-65, -64, -63, -17, -16, -15, -1, 0, 1, 15, 16, 17, 63, 64, 65]


def structure_grid():
    """Yields (label, block, capacity, payload): valid blocks, one per structural threshold of lzd_block and side of it."""
    count = [0]

    def emit(label, b, tail=12, room=None):
        block, payload = b.end(tail)
        count[0] += 1
        extra = (0, 64, 0, 17)[count[0] % 4] if room is None else room      # capacity exact, and with room behind the payload
        return label, block, len(payload) + extra, payload

    # (1) the 64-byte look-ahead in registers (`lv`, in_u8) and the fast path's `jo + 2 <= la_n`: token, every length byte,
    #     both offset bytes land on both sides of a 64-byte step of the look-ahead;
    # (2) the 4 KiB input window (kLzdWin, refill): the same around the first window's end and around the second one's
    sweeps = list(range(0, 71)) + list(range(4030, 4101)) + list(range(8126, 8201))
    for style, fixed in (("lit", "b"), ("fast", "a"), ("fast", "c"), ("short", "b")):
        for p in sweeps:
            if style != "lit" and p in (1, 2):                              # (no sequence has fewer than 3 bytes)
                continue
            b = _lead_in(style, p)
            ll, ml = _FIXED[fixed]
            b.seq(ll, 1 + p % 23, ml)
            b.seq(2, 2 + p % 5, 9)              # (a fast-path sequence behind it: the state the general path leaves)
            yield emit(f"lookahead/{style}/{fixed}/p{p}", b)
    # runs of 255-valued length bytes across the window's edge: 13 length bytes that start at input byte q
    for q in range(4026, 4100, 3):
        for which in ("literal", "match"):
            b = _lead_in("fast", q - 10)        # (the lead-in's first sequence has 10 bytes: the token below is input byte q)
            assert len(b.blk) == q
            if which == "literal":
                b.seq(15 + 255 * 12 + 5, 700, 7)
            else:
                b.seq(3, 2, 4 + 15 + 255 * 12 + 5)
            b.seq(1, 1000, 40)
            yield emit(f"length_bytes_at_window_edge/{which}/q{q}", b)
    # (3) kLzdShortLit = 512 (window copy | direct global copy), the direct copy's 8192 bytes per loop trip, kLzdPiece: literal
    #     runs that start at input residues 0, 3, 50, 60 (mod 64), as a sequence's literals and as the block's last literals
    for run in _LIT_RUNS:
        n_len = 0 if run < 15 else 1 + (run - 15) // 255
        for res in (0, 3, 50, 60):
            k = next(k for k in range(1, 90) if (len(_seq(bytes(k), 1, 4)) + 1 + n_len) % 64 == res)
            b = _Builder().seq(k, 1, 4).seq(run, 1 + run % 9, 5)
            yield emit(f"literal_run/{run}/res{res}/middle", b)
            b = _Builder().seq(k, 1, 4)
            yield emit(f"literal_run/{run}/res{res}/last", b, tail=run)
    # (4) kLzdPiece = 16384 and the periodic copy's restart per piece (`start = v0 - off`, r0, s64): every offset below 64;
    # (5) offset < 64 (periodic) | offset >= 64 (64 bytes per step), the reciprocal-based lane mod off
    for off in list(range(1, 71)) + [127, 128, 129]:
        for ml in _LONG_ML:
            b = _Builder().seq(off + off % 5, off, ml)
            b.seq(3, min(ml // 2 + off, 65535), 21)                         # (reads the match back: the ring behind it is whole)
            yield emit(f"long_match/off{off}/ml{ml}", b)
    for off in range(1, 71):                                                # the fast path's match lengths, 4..18
        b = _Builder().seq(off, off, 19)
        for ml in range(4, 19):
            b.seq(2 + ml % 3, off, ml)
        yield emit(f"fast_match_lengths/off{off}", b)
    # (6) the 64-lane read-then-write step with an offset next to the ring's size: every offset 65472..65535
    for off in range(65472, 65536):
        for ml in (64, 128, 129, 16385):
            b = _Builder().seq(65536 + 100 - 4, 9, 4)
            b.seq(0, off, ml)
            b.seq(1, off, 6)
            yield emit(f"far_offset/off{off}/ml{ml}", b)
    # (7) the 64 KiB ring's wrap (kLzdMask): a history that ends d bytes from a multiple of the ring, then each kind of copy
    for base in (65536, 131072):
        for d in _WRAP_D:
            for what in ("short_literals", "long_literals", "periodic", "far", "fast_chain"):
                b = _Builder().seq(base + d - 4, 100, 4)
                if what == "short_literals":
                    b.seq(140, 33, 8)
                elif what == "long_literals":
                    b.seq(5000, 33, 8)
                elif what == "periodic":
                    b.seq(1, 7, 300)
                elif what == "far":
                    b.seq(1, 60000, 500)
                else:
                    b.fast_chain(130)
                b.seq(2, 65000, 150)
                yield emit(f"ring_wrap/{base}{d:+d}/{what}", b)
    # (8) kLzdDrainAt = 32768: the fast path's own `out + a - drained < kLzdDrainAt`, literals written out of the look-ahead
    #     without a look at the drain mark
    #     (sequences WITHOUT literals matter most: literals that straddle the look-ahead's end go through copy_literals, which
    #     drains by itself; behind a run of literal-free sequences only the match copy's look at the drain mark is left)
    for ll, off, ml in ((3, 5, 12), (14, 20000, 18), (0, 3, 4), (0, 2, 18), (7, 64, 17)):
        first = 20000 if off > 100 else max(ll, 8, off)
        b = _Builder().seq(first, first, 5)                                 # (a history that is not one byte repeated)
        target = len(b.out) + 100000                                        # (the ring goes round as well)
        while len(b.out) < target:
            b.seq(ll, off, ml)
        yield emit(f"drain/fast_path_only/ll{ll}_off{off}_ml{ml}", b)
    for k in range(0, 71):
        for name, ml in (("general", 40), ("fast", 8)):
            b = _Builder().seq(32768 - k - 4, 9, 4)
            assert len(b.out) == 32768 - k
            b.seq(10, 31000, ml)
            b.seq(5, 3, 100)
            yield emit(f"drain/lookahead_literals_at_32768-{k}/{name}", b)
    # (9) the end of the block (`ip + ll + 9 <= n_in`, `o1 + 12 <= cap`, `o1 + ml + 5 <= cap`): the accepted side of each
    #     (reject_table() has the other side) -- a last match that ends exactly 5 bytes in front of the capacity, behind it the
    #     shortest tail there is, at the exact capacity and with 64 bytes to spare. (A final sequence WITHOUT literals exists
    #     only as the block 00: behind a match the rules want 5 literals, `ip > iend - 4` refuses anything shorter; the block 00
    #     is in reject_table() at capacity 0 and 64 and is every guard span of the device tests.)
    for ml in (7, 8, 18, 19, 20, 64, 300):
        for ll in (0, 1, 13):
            for room in (0, 64):
                b = _Builder().seq(8, 8, 4).seq(ll, 3, ml)
                yield emit(f"end/last_match_{ml}_behind_{ll}_literals/tail5/room{room}", b, tail=5, room=room)


def damaged_grid_sample(every: int = 3, max_block: int = 12000, trials: int = 4):
    """[(label, block, capacity)]: every `every`-th grid block of at most max_block bytes, damaged `trials` ways (fixed seeds)."""
    out = []
    for k, (label, block, cap, _payload) in enumerate(structure_grid()):
        if k % every or len(block) > max_block:
            continue
        rs = np.random.RandomState(k)
        for t in range(trials):
            out.append((f"{label}/damage{t}", damaged(rs, block), cap))
    return out
