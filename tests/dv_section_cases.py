"""The case table of tests/test_dv_section_cases.py (CPU) and tests/test_gpu_dv_sections.py: chunks whose DeltaVarint SECTIONS (mode
byte 0 of decodeV5AdaptiveIntSection) are built from CHOSEN token lengths, for the tile walker behind k_decode_sections, k_decode_tail
and k_decode_sections_cols (dv_stream with one 64-bit integer op, stage1_decode.h). The oracle's encoder writes every stream:
Oracle.encode_stage1_continued forces the section modes. Every row carries a predicate on the parsed stream that proves the row is what
its name says; the CPU test evaluates it against the oracle's bytes. DESIGN.md section 4 ("The DeltaVarint section grid") has the table
in words.

Token lengths are chosen through the deltas: the token of a delta d is the varint of zigzag(d) + 1, so d = +-2^(7(L-1)-1) (0 for L = 1)
gives exactly L bytes, for every L = 1..10, and a 64-bit field wraps like the decoder's sum does. The walker's tile is TILE bytes
counted from the section's first token byte (the byte behind the mode byte).
"""
from __future__ import annotations

import numpy as np

import cases

F = cases.F
TILE = 8192
CHUNK = 32768
M64 = (1 << 64) - 1
_SIZE = {F.UINT16: 2, F.UINT32: 4, F.UINT64: 8, F.INT64: 8}
_XYZ = [("x", 0, F.FLOAT32, 0.001), ("y", 4, F.FLOAT32, 0.001), ("z", 8, F.FLOAT32, 0.001)]

# name -> (fields, point step, tokens of the regular stream per point, the kernel whose DeltaVarint arm decodes the sections and why)
SCHEMAS = {
    # no regular op, one 8-byte field: bpv 8 fails narrow_fields -> DS_SMALL_GENERAL; k_decode_sections_small steps aside (mode byte 0)
    "U64": ([("v", 0, F.UINT64, None)], 8, 0, "k_decode_sections"),
    "I64": ([("v", 0, F.INT64, None)], 8, 0, "k_decode_sections"),
    # two fields, one of 8 bytes: the same route; the section modes take turns with the LDS of one workgroup
    "U64_U32": ([("v", 0, F.UINT64, None), ("w", 8, F.UINT32, None)], 12, 0, "k_decode_sections"),
    "U32_U64": ([("w", 0, F.UINT32, None), ("v", 4, F.UINT64, None)], 12, 0, "k_decode_sections"),
    # XYZ -> DR_POINTS; one field, but of 8 bytes: no columns, the point kernel folds small Palettes only -> k_decode_tail
    "XYZ_U64": (_XYZ + [("v", 12, F.UINT64, None)], 20, 3, "k_decode_tail"),
    # XYZ + two narrow fields -> DC_COLS; two fields, so no k_sections_cols_fast: dense columns of 2- and 4-byte values
    "XYZ_U16_U32": (_XYZ + [("v", 12, F.UINT16, None), ("w", 14, F.UINT32, None)], 20, 3, "k_decode_sections_cols"),
    "XYZ_U16_U32_STEP19": (_XYZ + [("v", 12, F.UINT16, None), ("w", 14, F.UINT32, None)], 19, 3, "k_decode_sections_cols"),
}


def deltas_for(lens):
    """uint64 deltas (two's complement) whose tokens have the lengths `lens`: +2^(7(L-1)-1) at even places, - at odd ones."""
    ln = np.asarray(lens, dtype=np.int64)
    assert ln.size and ln.min() >= 1 and ln.max() <= 10
    mag = np.where(ln == 1, np.uint64(0), np.uint64(1) << (7 * (ln - 1) - 1).clip(0).astype(np.uint64)).astype(np.uint64)
    neg = (np.arange(ln.size) & 1).astype(bool)
    return np.where(neg, (~mag + np.uint64(1)).astype(np.uint64), mag)


def values_for(lens):
    """uint64 field values whose DeltaVarint tokens have the lengths `lens` (sums modulo 2^64)."""
    with np.errstate(over="ignore"):
        return np.cumsum(deltas_for(lens), dtype=np.uint64)


def varint_len(x):
    n = 1
    while x >> (7 * n):
        n += 1
    return n


# ---------------------------------------------------------------------------------------------------------------------
# parsing what the oracle wrote
# ---------------------------------------------------------------------------------------------------------------------
def split_chunks(stream):
    """[(payload offset in the stream, payload)]"""
    s, pos, out = np.asarray(stream, dtype=np.uint8), 0, []
    while pos < len(s):
        size = int(np.frombuffer(s[pos:pos + 4].tobytes(), "<u4")[0])
        out.append((pos + 4, s[pos + 4:pos + 4 + size]))
        pos += 4 + size
    return out


def frame(payloads):
    return np.concatenate([np.concatenate([np.frombuffer(np.uint32(len(p)).tobytes(), np.uint8), np.frombuffer(bytes(p), np.uint8)])
                           for p in payloads])


def _tokens(p, pos, count):
    """lengths of `count` varint tokens from byte pos on, and the offset behind them"""
    ends = np.nonzero((p[pos:] & 0x80) == 0)[0][:count]
    assert len(ends) == count
    return np.diff(np.concatenate([[-1], ends])), pos + int(ends[-1]) + 1 if count else pos


class Section:
    def __init__(self, mode, start, end, lens=None, count=0):
        self.mode, self.start, self.end, self.lens, self.count = mode, start, end, lens, count   # start: the byte behind the mode byte


class Parsed:
    def __init__(self, payload, reg_end, sections):
        self.payload, self.reg_end, self.sections = payload, reg_end, sections


def parse_chunk(payload, n, reg_tokens, bpvs):
    p = np.asarray(payload, dtype=np.uint8)
    _l, pos = _tokens(p, 0, n * reg_tokens) if reg_tokens else (None, 0)
    reg_end, secs = pos, []
    for bpv in bpvs:
        mode = int(p[pos])
        pos += 1
        start, lens, count = pos, None, 0
        if mode == 0:
            lens, pos = _tokens(p, pos, n)
        elif mode == 1:
            count = int(p[pos]) | (int(p[pos + 1]) << 8)
            bits = 0 if count <= 1 else int(count - 1).bit_length()
            pos += 2 + count * bpv + (bits * n + 7) // 8
        else:
            count = int.from_bytes(p[pos:pos + 4].tobytes(), "little")
            pos += 4
            for _r in range(count):
                if mode == 2:
                    pos += bpv
                else:
                    pos = _tokens(p, pos, 1)[1]
                pos = _tokens(p, pos, 1)[1]
        secs.append(Section(mode, start, pos, lens, count))
    assert pos == len(p), (pos, len(p))
    return Parsed(p, reg_end, secs)


# ---------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, name, family, schema, cols, modes, pred, note="", damage=None, error=None):
        self.name, self.family, self.schema, self.cols, self.modes, self.pred, self.note = name, family, schema, cols, list(modes), pred, note
        self.fields, self.step, self.reg_tokens, self.kernel = SCHEMAS[schema]
        self.n = len(next(iter(cols.values())))
        self.ns = [CHUNK] * ((self.n - 1) // CHUNK) + [self.n - (self.n - 1) // CHUNK * CHUNK]
        self.bpvs = [_SIZE[f[2]] for f in self.fields if f[3] is None]
        self.damage = damage      # malformed rows: payload bytes -> payload bytes of the one chunk
        self.error = error        # ... and the oracle's error code (ORC_ERR_TRUNCATED -4 / ORC_ERR_CORRUPT -5)
        assert len(self.modes) == len(self.bpvs)

    def info(self):
        return cases.make_info(self.fields, self.step, self.n)

    def cloud(self):
        cols = dict(self.cols)
        for f in self.fields[:self.reg_tokens]:
            cols.setdefault(f[0], np.zeros(self.n, dtype=np.float32))     # a cloud that stands still at 0: every token the byte 0x01
        return cases.pack(self.info(), cols, self.n)

    def stream(self, oracle):
        s = oracle.encode_stage1_continued(self.info(), self.cloud(), self.modes)
        if self.damage is not None:
            (_off, payload), = split_chunks(s)
            s = frame([self.damage(self.parse(s)[0])])
        return s

    def parse(self, stream):
        return [parse_chunk(p, n, self.reg_tokens, self.bpvs) for (_o, p), n in zip(split_chunks(stream), self.ns)]


# ---- predicates: pred(P) with P = row.parse(stream), one Parsed per chunk
def dv(P, chunk=0, k=None):
    """the (k-th, default: only) DeltaVarint section of a chunk"""
    secs = [s for s in P[chunk].sections if s.mode == 0]
    assert k is not None or len(secs) == 1
    return secs[k or 0]


def lens_are(lens, chunk=0):
    return lambda P: dv(P, chunk).lens.tolist() == list(lens)


def token_ends_on(byte, chunk=0):
    """a token's last byte is byte `byte` of the section (tile byte `byte` % TILE of tile `byte` // TILE)"""
    return lambda P: byte in (np.cumsum(dv(P, chunk).lens) - 1)


def ten_bytes_across(edge, k):
    """a 10-byte token begins k bytes in front of section byte `edge`"""
    def pred(P):
        ends = np.cumsum(dv(P).lens)
        i = int(np.searchsorted(ends, edge - k + 10))
        return ends[i] == edge - k + 10 and dv(P).lens[i] == 10
    return pred


def section_bytes(size_mod8=None, size=None):
    def pred(P):
        s = dv(P)
        return (size is None or s.end - s.start == size) and (size_mod8 is None or (s.end - s.start) % 8 == size_mod8)
    return pred


def modes_are(modes, counts=None):
    return lambda P: all([s.mode for s in c.sections] == list(modes) for c in P) and \
        (counts is None or all(lo <= s.count <= hi for c in P for s, (lo, hi) in zip(c.sections, counts)))


def both(*preds):
    return lambda P: all(p(P) for p in preds)


# ---------------------------------------------------------------------------------------------------------------------
def _u64(lens, schema="U64"):
    v = values_for(lens)
    return {"v": v.view(np.int64) if schema == "I64" else v}


def _cycle(n, start=0):
    return [(start + i) % 10 + 1 for i in range(n)]


def _narrow(n, dtype):
    """a 16- / 32-bit field whose deltas wrap the value: steps of +-(2^bits - 1 - small), tokens of 3 / 5 bytes"""
    bits = 8 * np.dtype(dtype).itemsize
    i = np.arange(n, dtype=np.int64)
    return np.where(i & 1, (1 << bits) - 1 - (i % 7), i % 5).astype(dtype)


def _palette(n, distinct):
    return ((np.arange(n, dtype=np.int64) * 2654435761 >> 7) % distinct * 3 + 1).astype(np.uint32)


def _runs(n):
    return np.repeat(np.arange((n + 36) // 37, dtype=np.uint32) * 5 % 11, 37)[:n]


def _ramps(n):
    return (np.arange(n, dtype=np.uint32) // 50 * 1000 + np.arange(n, dtype=np.uint32) % 50 * 3).astype(np.uint32)


def _damage_token(index, new):
    """replace token `index` (negative: from the end) of the section by the bytes `new`"""
    def fn(P):
        s = dv([P])
        ends = s.start + np.cumsum(s.lens)
        i = index % len(ends)
        a = s.start if i == 0 else int(ends[i - 1])
        return np.concatenate([P.payload[:a], np.frombuffer(bytes(new), np.uint8), P.payload[int(ends[i]):]])
    return fn


def _table():
    T = []
    # ---- a: every token length, uniform, on both 64-bit types; one row cycles through all ten
    for s in ("U64", "I64"):
        for L in range(1, 11):
            n = 5000
            T.append(Row("a_len%d_%s" % (L, s), "a", s, _u64([L] * n, s), [0], both(lens_are([L] * n), section_bytes(size=n * L))))
    T.append(Row("a_lengths_cycle", "a", "U64", _u64(_cycle(5000)), [0], lens_are(_cycle(5000))))
    # ---- b: the tile edges, section bytes 8192 and 16384 (the lengths of the tokens in front are chosen)
    tail = [3, 1, 5, 2, 10, 1, 7] * 6
    T.append(Row("b_token_ends_on_tile_byte_8191", "b", "U64", _u64([1] * (TILE - 2) + [2] + tail), [0],
                 both(token_ends_on(TILE - 1), lambda P: dv(P).lens[TILE - 2] == 2)))
    T.append(Row("b_token_ends_on_tile_byte_8192", "b", "U64", _u64([1] * (TILE - 1) + [2] + tail), [0],
                 both(token_ends_on(TILE), lambda P: dv(P).lens[TILE - 1] == 2 and not token_ends_on(TILE - 1)(P))))
    for k in range(1, 10):
        T.append(Row("b_ten_bytes_%d_in_front_of_the_first_edge" % k, "b", "U64", _u64([1] * (TILE - k) + [10] + tail), [0],
                     ten_bytes_across(TILE, k)))
    for k in range(1, 10):
        T.append(Row("b_ten_bytes_%d_in_front_of_the_second_edge" % k, "b", "U64", _u64([2] * (TILE // 2) + [1] * (TILE - k) + [10] + tail), [0],
                     ten_bytes_across(2 * TILE, k)))
    # ---- c: the partial last 8-byte unit (the byte-wise load): section sizes 0..7 (mod 8), the last token 10 bytes
    for r in range(8):
        lens = [4] * 250 + [1] * ((r - 10 - 1000) % 8) + [10]
        T.append(Row("c_section_bytes_%d_mod_8" % r, "c", "U64", _u64(lens), [0], section_bytes(size_mod8=r)))
    # ---- d: a section at every residue (mod 8) of the payload: 1..8 points of a cloud that stands still, 3 bytes each, in front
    for n in range(1, 9):
        T.append(Row("d_section_at_residue_%d" % ((3 * n + 1) % 8), "d", "XYZ_U64", _u64(_cycle(n, start=6)), [0],
                     lambda P, n=n: P[0].reg_end == 3 * n and dv(P).start % 8 == (3 * n + 1) % 8))
    # ---- e: counts
    T.append(Row("e_n1", "e", "U64", _u64([10]), [0], lens_are([10])))
    T.append(Row("e_n2", "e", "U64", _u64([9, 10]), [0], lens_are([9, 10])))
    T.append(Row("e_four_tiles_exactly", "e", "U64", _u64([1] * CHUNK), [0], section_bytes(size=4 * TILE)))
    T.append(Row("e_forty_tiles", "e", "U64", _u64([10] * CHUNK), [0], section_bytes(size=40 * TILE)))
    T.append(Row("e_two_chunks", "e", "U64", _u64(_cycle(CHUNK + 1)), [0],
                 lambda P: len(P) == 2 and dv(P, 0).lens.tolist() == _cycle(CHUNK) and len(dv(P, 1).lens) == 1))
    # ---- f: neighbours in one chunk (LDS reuse between the arms of decode_sections_core and the barrier between them)
    n = 9000
    lens = _cycle(n)
    other = {0: values_for(_cycle(n, 3)).astype(np.uint32), 1: _palette(n, 7), 2: _runs(n), 3: _ramps(n)}
    for m in (0, 1, 3, 2):
        T.append(Row("f_dv_then_mode%d" % m, "f", "U64_U32", {"v": values_for(lens), "w": other[m]}, [0, m], modes_are([0, m])))
        if m:
            T.append(Row("f_mode%d_then_dv" % m, "f", "U32_U64", {"w": other[m], "v": values_for(lens)}, [m, 0], modes_are([m, 0])))
    # more than 1024 entries: k_decode_sections_small steps aside at the Palette too
    T.append(Row("f_dv_then_large_palette", "f", "U64_U32", {"v": values_for(lens), "w": _palette(n, 2000)}, [0, 1],
                 modes_are([0, 1], [(0, 0), (1025, 4096)])))
    T.append(Row("f_large_palette_then_dv", "f", "U32_U64", {"w": _palette(n, 2000), "v": values_for(lens)}, [1, 0],
                 modes_are([1, 0], [(1025, 4096), (0, 0)])))
    # ---- g: the other two kernels that run the arm
    n = 20000
    T.append(Row("g_tail_xyz_u64", "g", "XYZ_U64", _u64(_cycle(n)), [0], lens_are(_cycle(n))))
    for s in ("XYZ_U16_U32", "XYZ_U16_U32_STEP19"):
        v, w = _narrow(n, np.uint16), _narrow(n, np.uint32)
        T.append(Row("g_cols_dv_dv_" + s, "g", s, {"v": v, "w": w}, [0, 0],
                     both(modes_are([0, 0]), lambda P: 3 in P[0].sections[0].lens and 5 in P[0].sections[1].lens)))
        T.append(Row("g_cols_dv_palette_" + s, "g", s, {"v": v, "w": _palette(n, 300)}, [0, 1], modes_are([0, 1])))
    # ---- h: malformed: a well-formed row with one place changed; the oracle's error code
    good = [4] * 250 + [1] * 5 + [10]
    for name, fn, err in (
            ("overlong_zero_for_a_token", _damage_token(100, [0x80, 0x00]), -5),
            ("lone_zero_byte_for_a_token", _damage_token(100, [0x00]), -5),
            ("token_of_11_bytes", _damage_token(100, [0x81] + [0x80] * 9 + [0x01]), -5),
            ("tenth_byte_with_two_value_bits", _damage_token(-1, [0x81] + [0x80] * 8 + [0x03]), -5),
            ("payload_cut_inside_the_last_token", lambda P: P.payload[:-4], -4),
            ("payload_cut_one_token_short", lambda P: P.payload[:-10], -4),
            ("one_byte_behind_the_last_section", lambda P: np.concatenate([P.payload, np.array([0x01], np.uint8)]), -5)):
        T.append(Row("h_" + name, "h", "U64", _u64(good), [0], None, damage=fn, error=err))
    T.append(Row("h_overlong_zero_behind_xyz", "h", "XYZ_U64", _u64(good), [0], None, damage=_damage_token(7, [0x80, 0x80, 0x00]), error=-5))
    return T


def rejected_by_its_own_decoder():
    """An INT64 field alternating 0 and INT64_MIN, forced to DeltaVarint: the deltas are +-2^63 = INT64_MIN both ways, whose token
    the encoder writes and no decoder takes. (cloud info, cloud, modes)"""
    n = 64
    v = np.where(np.arange(n) & 1, np.int64(-(1 << 63)), np.int64(0)).astype(np.int64)
    info, data = cases.int_only(v, F.INT64)
    return info, data, [0]


REFERENCE_REJECTS_INT64_MIN_DELTAS = True   # proved against the compiled reference by tests/test_dv_section_cases.py

ROWS = _table()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS) and len(ROWS) <= 120
WELL_FORMED = [r for r in ROWS if r.error is None]
MALFORMED = [r for r in ROWS if r.error is not None]
