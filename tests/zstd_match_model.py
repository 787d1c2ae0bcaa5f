"""Serial restatement of the device ZSTD writer with the matches switch on (cloudini_amd/csrc/zstd_seq_kernels.hip,
cldn_hip_codec_set_zstd_matches): frames whose blocks may hold sequences.

It builds on zstd_lit_model.py (Huffman lengths, code values, tree descriptions, stream bytes) and on the LZ4 model's matches
(Oracle.lz4_trace with the standard parameters: 8192-byte sub-ranges, 11 hash bits, 1024 matches per sub-range). Sixteen
sub-ranges are one 128 KiB block and a match never leaves its sub-range, so never its block.

The choices that are this writer's own, and that the kernels restate:
  * a block's kept matches are those of its sub-ranges with len >= MIN_MATCH, in position order; a block without one, and a
    block of fewer than 64 bytes, is zstd_lit_model.block's, byte for byte
  * a block with kept matches is Compressed: a literals section over the bytes no kept match covers (fewer than 64 of them:
    Raw literals; one byte value: RLE literals; else Huffman by zstd_lit_model's rules, one stream below 256 literals and four
    from there on, unless header + streams would not be smaller than the Raw literals section), the sequence count (1 byte
    below 128, else 2), the modes byte 0x00 (Predefined tables), and the backward bit stream
  * the offset value is off + 3, never a repeat code
  * the bit stream is what the format's reference encoder lays down: the three states start at the last sequence's codes, at
    the cell init_state() fixes; the last sequence's extra bits (literal length, match length, offset) come first in memory;
    every earlier sequence, last to first, adds the state bits of offset, match length and literal length and then its extra
    bits; the states (match length, offset, literal length) and the final 1 bit close it
  * if the Compressed form is not smaller than the block, the block is Raw
"""
from __future__ import annotations

import numpy as np

import zstd_lit_model as L
from zstd_lit_model import BLOCK, HUF, MIN_HUF, RAW, RLE

SUB = 8192
HASH_BITS = 11
MAX_MATCHES = 1024
SUBS_PER_BLOCK = BLOCK // SUB
MAX_SEQ = SUBS_PER_BLOCK * MAX_MATCHES      # 16384 < 0x7F00: the 3-byte sequence count is out of reach
MIN_MATCH = 12                       # kZsMinMatch (zstd_seq_code.h); chosen by test_zstd_match_model.py's size table
CANDIDATES = (4, 5, 6, 8, 12)

LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
LL_LOG, ML_LOG, OF_LOG = 6, 6, 5

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        from oracle import binding
        binding.build()
        _oracle = binding.Oracle()
    return _oracle


# ---- codes and extra bits ----------------------------------------------------------------------------------------------------------
def highbit(v: int) -> int:
    return int(v).bit_length() - 1


def ll_code(ll: int) -> int:
    if ll < 16:
        return ll
    if ll < 24:
        return 16 + ((ll - 16) >> 1)
    if ll < 32:
        return 20 + ((ll - 24) >> 2)
    if ll < 48:
        return 22 + ((ll - 32) >> 3)
    if ll < 64:
        return 24
    return highbit(ll) + 19


def ll_bits(code: int) -> int:
    return 0 if code < 16 else 1 if code < 20 else 2 if code < 22 else 3 if code < 24 else 4 if code == 24 else code - 19


def ml_code(mb: int) -> int:
    """mb = match length - 3"""
    if mb < 32:
        return mb
    if mb < 40:
        return 32 + ((mb - 32) >> 1)
    if mb < 48:
        return 36 + ((mb - 40) >> 2)
    if mb < 64:
        return 38 + ((mb - 48) >> 3)
    if mb < 96:
        return 40 + ((mb - 64) >> 4)
    if mb < 128:
        return 42
    return highbit(mb) + 36


def ml_bits(code: int) -> int:
    return 0 if code < 32 else 1 if code < 36 else 2 if code < 38 else 3 if code < 40 else 4 if code < 42 else 5 if code == 42 else code - 36


# the format's tables (RFC 8878, 3.1.1.3.2.1.1), to hold the arithmetic above against
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


# ---- FSE encoding tables of the predefined distributions ---------------------------------------------------------------------------
class CTable:
    """delta_nb / delta_state per symbol and the state table, as the reference encoder builds them"""

    def __init__(self, norm, log):
        size = 1 << log
        self.log = log
        step = (size >> 1) + (size >> 3) + 3
        cell = [0] * size
        high = size - 1
        for s, c in enumerate(norm):                       # the "less than 1" symbols take the top cells, the first the highest
            if c == -1:
                cell[high] = s
                high -= 1
        pos = 0
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                cell[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0
        cum = [0]
        for c in norm:
            cum.append(cum[-1] + abs(c))
        fill = list(cum)
        self.state = [0] * size
        for u in range(size):
            self.state[fill[cell[u]]] = size + u
            fill[cell[u]] += 1
        self.delta_nb, self.delta_state = [], []
        total = 0
        for c in norm:
            c = abs(c)
            if c == 1:
                self.delta_nb.append((log << 16) - size)
                self.delta_state.append(total - 1)
            else:
                out = log - highbit(c - 1)
                self.delta_nb.append((out << 16) - (c << out))
                self.delta_state.append(total - c)
            total += c

    def init_state(self, sym: int) -> int:
        nbo = (self.delta_nb[sym] + 32768) >> 16
        v = (nbo << 16) - self.delta_nb[sym]
        return self.state[(v >> nbo) + self.delta_state[sym]]

    def step(self, state: int, sym: int):
        """-> (bits written, their number, next state)"""
        nbo = (state + self.delta_nb[sym]) >> 16
        return state & ((1 << nbo) - 1), nbo, self.state[(state >> nbo) + self.delta_state[sym]]


LL_T, ML_T, OF_T = CTable(LL_NORM, LL_LOG), CTable(ML_NORM, ML_LOG), CTable(OF_NORM, OF_LOG)


def sequence_fields(ll: int, ml: int, off: int):
    """-> (ll code, ml code, of code, [(value, bits)] of the extra bits in stream order)"""
    lc, mc = ll_code(ll), ml_code(ml - 3)
    ov = off + 3
    oc = highbit(ov)
    assert LL_BASE[lc] <= ll and ll - LL_BASE[lc] < (1 << LL_BITS[lc]) == (1 << ll_bits(lc))
    assert ML_BASE[mc] <= ml and ml - ML_BASE[mc] < (1 << ML_BITS[mc]) == (1 << ml_bits(mc))
    extra = [(ll & ((1 << ll_bits(lc)) - 1), ll_bits(lc)), ((ml - 3) & ((1 << ml_bits(mc)) - 1), ml_bits(mc)), (ov & ((1 << oc) - 1), oc)]
    assert extra[0][0] == ll - LL_BASE[lc] and extra[1][0] == ml - ML_BASE[mc]
    return lc, mc, oc, extra


def sequence_bits(seqs, note=None) -> bytes:
    """seqs: rows (literal length, match length, offset), first to last -> the bit stream. note["pieces"]: bits per sequence in
    memory order (the last sequence first), then the 18 closing bits"""
    b = L.Bits()
    pieces = []
    st = None
    for ll, ml, off in reversed([tuple(int(x) for x in r) for r in seqs]):
        lc, mc, oc, extra = sequence_fields(ll, ml, off)
        at = b.n
        if st is None:
            st = [OF_T.init_state(oc), ML_T.init_state(mc), LL_T.init_state(lc)]
        else:
            for k, (t, sym) in enumerate(((OF_T, oc), (ML_T, mc), (LL_T, lc))):
                v, nb, st[k] = t.step(st[k], sym)
                b.add(v, nb)
        for v, nb in extra:
            b.add(v, nb)
        pieces.append(b.n - at)
    b.add(st[1], ML_LOG)
    b.add(st[0], OF_LOG)
    b.add(st[2], LL_LOG)
    b.add(1, 1)
    if note is not None:
        note["pieces"] = pieces
        note["seq_bits"] = b.n
    return b.bytes()


# ---- blocks ------------------------------------------------------------------------------------------------------------------------
def raw_literals_header(kind: int, n: int) -> bytes:
    """Raw (0) or RLE (1) literals of n bytes"""
    if n < 32:
        return bytes([kind | (n << 3)])
    if n < 4096:
        return (kind | (1 << 2) | (n << 4)).to_bytes(2, "little")
    return (kind | (3 << 2) | (n << 4)).to_bytes(3, "little")


def literals_section(lits: np.ndarray, note):
    """-> bytes. note: lit_kind, lit_form, lit_streams"""
    n = lits.size
    raw = raw_literals_header(0, n) + lits.tobytes()
    note.update(n_lit=n, lit_kind=RAW, lit_form=None, lit_streams=0)
    if n < MIN_HUF:
        return raw
    counts = np.bincount(lits, minlength=256)
    if np.count_nonzero(counts) == 1:
        note["lit_kind"] = RLE
        return raw_literals_header(1, n) + lits[:1].tobytes()
    lens = L.code_lengths(counts)
    codes, max_len = L.code_values(lens)
    desc = L.tree_description(lens, max_len)
    if desc is None:
        return raw
    four = n >= L.FOUR_STREAMS
    if four:
        seg = (n + 3) // 4
        streams = [L.stream_bytes(lits[k * seg:min(n, (k + 1) * seg)], lens, codes) for k in range(4)]
        jump = b"".join(len(s).to_bytes(2, "little") for s in streams[:3])
    else:
        streams, jump = [L.stream_bytes(lits, lens, codes)], b""
    comp = len(desc) + len(jump) + sum(len(s) for s in streams)
    if comp >= 262144:
        return raw
    hdr_size = 3 if (not four or (n < 1024 and comp < 1024)) else 4 if (n < 16384 and comp < 16384) else 5
    if hdr_size + comp >= len(raw):                       # nothing gained
        return raw
    form, hdr = L.literals_header(n, comp, four)
    note.update(lit_kind=HUF, lit_form=form, lit_streams=len(streams))
    return hdr + desc + jump + b"".join(streams)


def kept_matches(matches: np.ndarray, lo: int, hi: int, min_match: int) -> np.ndarray:
    """rows (pos, len, off) of the trace that start in [lo, hi) and are long enough"""
    if matches.shape[0] == 0:
        return matches
    sel = (matches[:, 0] >= lo) & (matches[:, 0] < hi) & (matches[:, 1] >= min_match)
    return matches[sel]


def block(data: np.ndarray, base: int, matches: np.ndarray, last: bool, note=None, min_match: int = MIN_MATCH) -> bytes:
    """data: the block, payload[base, base + n); matches: the chunk's trace rows"""
    note = {} if note is None else note
    n = data.size
    kept = kept_matches(matches, base, base + n, min_match) if n >= MIN_HUF else matches[:0]
    note.update(n_seq=0, matched=False)
    if kept.shape[0] == 0:
        return L.block(data, last, note)[2]
    assert kept.shape[0] <= MAX_SEQ < 0x7F00
    seqs, parts, at = [], [], base
    for pos, ln, off in kept.tolist():
        assert at <= pos and pos + ln <= base + n and 1 <= off <= pos - base
        seqs.append((pos - at, ln, off))
        parts.append(data[at - base:pos - base])
        at = pos + ln
    parts.append(data[at - base:])
    lits = np.concatenate(parts)
    note.update(n=n, kind=HUF, form=None, n_seq=len(seqs), trailing=base + n - at, seqs=seqs)
    lit = literals_section(lits, note)
    count = bytes([len(seqs)]) if len(seqs) < 128 else bytes([(len(seqs) >> 8) + 0x80, len(seqs) & 255])
    body = lit + count + b"\x00" + sequence_bits(seqs, note)
    note["body"] = len(body)
    if len(body) >= n:
        note.update(kind=RAW, why_raw="matches do not pay", n_seq=0)
        return L.block_header(last, RAW, n) + data.tobytes()
    note["matched"] = True
    return L.block_header(last, HUF, len(body)) + body


def frame_info(payload, trace=None, min_match: int = MIN_MATCH, lz=None):
    """-> frame bytes; trace (a list) takes block()'s note of every block; lz: the payload's Oracle.lz4_trace, if at hand"""
    data = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8).ravel()
    n = data.size
    if n == 0:
        return L.frame_info(data, trace)[0]
    if lz is None:
        lz = oracle().lz4_trace(data, SUB, HASH_BITS, MAX_MATCHES)
    matches = lz.matches.astype(np.int64)
    out = [b"\x28\xb5\x2f\xfd\xa0", n.to_bytes(4, "little")]
    for o in range(0, n, BLOCK):
        note = {}
        if trace is not None:
            trace.append(note)
        out.append(block(data[o:o + BLOCK], o, matches, o + BLOCK >= n, note, min_match))
        note["list_max"] = int(lz.subs["count"][o // SUB:(o + BLOCK) // SUB].max())   # the longest match list of its sub-ranges
    return b"".join(out)


def frame(payload, min_match: int = MIN_MATCH) -> bytes:
    return frame_info(payload, None, min_match)
