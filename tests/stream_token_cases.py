"""The case table of tests/test_stream_token_cases.py (CPU) and tests/test_gpu_stream_tokens.py: chunks whose regular stream is built
from CHOSEN token lengths at CHOSEN positions, for k_decode_stream_w (MODE 0 with MSB ends and with the marker kernels' bitmap, MODE 1)
and k_decode_fixed (cloudini_amd/csrc/stage1_decode_stream.h). The oracle's encoder writes every stream; every row carries a predicate
on the bytes it wrote that proves the row is what its name says. DESIGN.md section 4 ("The stream-decoder token grid") has the table
in words.

Token codes: 0 = the NaN marker (one byte 0x00, float ops only), L = 1..10 = a varint token of L bytes. Lengths are chosen through
the deltas: a lossy float lane at resolution 0.5, or an integer field on the version-4 wire, holds q = a running sum of deltas +-m(L)
whose token -- the varint of zigzag(delta) + 1 -- has exactly L bytes. The k-th token of a length class in a lane goes up for even k
and down for odd k. Narrow ops (FloatN lanes, Float_Lossy<float>, INT32) use m(L) = 2^(7(L-1)-1), L <= 5, which float32 holds exactly
(bits 6..27); Float_Lossy<float> also takes L = 6..10 where no other class is up at the same time. 64-bit ops (Float_Lossy<double>,
INT64) use m(L) = 2^(7L-2), and 2^62 for L = 10: bits 12..62, which a double holds exactly. Raw fields carry chosen bytes.

Positions are counted as the kernel's header comment counts them: v = payload offset + a0, a0 = the payload's address mod 16; piece p
is v in [1024 p, 1024 (p + 1)), sixty-four units of 16 bytes (lane = unit), a halo of six units behind it. MODE 0: the piece owns the
points that begin behind the token ends it holds (the point behind the end at byte 1023 begins in the halo, at 1024), piece 0 also
point 0. MODE 1: the piece owns the points whose first byte it holds. `Model` restates that in numpy and shares nothing with the
kernel's code path; the CPU test holds it against a byte-by-byte walk.

WHICH OBSERVABLE SAYS THAT THE STREAM KERNEL KEPT A CHUNK (read from the code at 837decf, not taken from the issue):

* `stream`: none. k_decode_stream_w writes reg_end[c] = kDecRedo for a chunk it gives up on (stage1_decode_stream.h, the block behind
  the last __syncthreads: `redo = misc[0] != 0 || pos == 0xffffffff`) and counts nothing; k_decode_varint<8, true> follows with
  redo_only = 1 (stage1_decode_route.h: `R.redo = DO_ANY; R.redo_only = stream_ok`), decodes the chunk, writes reg_end = the offset
  behind the last token and counts it under the same kStatFastRegular (stage1_decode.h, decode_varint_body: `reg_end[c] = redo ?
  kDecRedo : misc[1]; if (!redo) atomicAdd(&status[kStatFastRegular], 1u)`). decode_stats(), reg_end and sec_done are the same for a
  kept and for a redone chunk. The issue's reading of both places is right.
* `stream_cols` (the PINNED TWIN of every `stream` row: the same regular stream in front of one small UINT16 field): sec_done[c] == 2 and
  one count under kStatFastSections come only from the stream kernel's column merge (`merged = !redo && use_cols && reg_end_pre[c] ==
  pos`). A chunk it hands back keeps sec_done == 0 from the kernel's first lines; k_decode_sections_small then decodes the section and
  leaves sec_done == 1.
* `stream_bitmap`, `form`, `fixed`: no redo kernel follows (`R.redo` stays DO_NONE in that branch of decode_route). A handed-back
  chunk keeps reg_end == kDecRedo, k_decode_general decodes all of it and counts it under kStatSerialChunks (stage1_decode.h,
  `atomicAdd(&status[regular_done ? kStatSerialSections : kStatSerialChunks], 1u)`): decode_stats() == (chunks, s, 0, 0) and
  reg_end == the model's end say "kept".
* section mode: a section the stream kernel finishes adds one to the chunk's counter of finished sections (`if (!redo && pos ==
  src_size) atomicAdd(reg_end + c, 1u)`; the launch passes the counters, done_cnt, where the regular launch passes reg_end);
  k_sections_done writes sec_done = 1 and counts the chunk under kStatFastSections when all its sections are finished, the others go
  to k_decode_sections / k_decode_general and count under kStatSerialSections: stats[1] == chunks, stats[3] == 0, sec_done == 1.

WHAT THE ISSUE ASKS FOR AND NO PLAN OF THE C ABI REACHES (tests/test_decode_route.py rows 9_raw, xyz_raw4_long_points):
* the stream kernel's `fixed_F` path outside section mode: an all-raw plan of at most 8 fields goes to k_decode_fixed, one of 9 or more
  has varint_and_raw == 0 (cldn_hip_plan_create wants 1..8 ops) and goes to the serial decoder. ALL_RAW_9 pins that route.
* k_mark_token_ends in front of the stream kernel: `automaton || form` holds for every plan with stream_ok and a varint op, so the
  marker is only chosen together with k_decode_varint (DR_MIXED_VARINT), for points beyond kSwMaxPointBytes, which no plan of 8 ops has.
* a raw field of 2 bytes between varints: 16-bit integers are varint ops (version 4, LOSSLESS) or sections (version 5); only
  EncodingOptions::NONE copies them, and then every field is raw.
* "two QF32 lanes", "five QF32 lanes": the fused FloatN encoder takes three or four leading lossy floats (LeadingLossyFloatFieldCount);
  two or five of them are scalar Float_Lossy<float> ops (F2, F5), whose tokens have up to 10 bytes and whose sums are 64-bit. QF32 ops
  reach the stream kernel next to other ops (XYZ_D, XYZ_D_F, XYZ_R4, ...). Likewise "3 QF32 + a lossy FLOAT32" alone would be four
  FloatN lanes (the point kernel's): XYZ_D_F puts a lossy FLOAT64 between them.
* section mode on 64-bit integer fields (tokens of 1 to 10 bytes): decode_route's narrow_fields wants bpv <= 4 for the side-by-side
  route, a plan with an 8-byte field takes k_decode_sections_small / k_decode_sections (tests/dv_section_cases.py owns those). The
  section rows here have tokens of 1 to 3 bytes (UINT16) and 1 to 5 bytes (UINT32).
* a form above kSwMaxPointBytes within 8 ops: 8 x 10 bytes stay below it; nine ops go to the serial decoder (ROUTE_ONLY).

HANDBACK is empty: a point of these routes has at most 8 ops of at most 10 bytes (80 <= kSwMaxPointBytes), tokens of 10 bytes are
well-formed for every op the stream kernel takes (a narrow op keeps the low 32 bits, as the serial decoder does), and a marker on an
integer op or a zero spread over several bytes is malformed (tests/test_gpu_malformed.py owns those).
"""
from __future__ import annotations

import numpy as np

import cases
import points_token_cases as PC
from cloudini_amd.schema import EncodingOptions

F = cases.F
PIECE, UNIT, UNITS, HALO, RING = 1024, 16, 64, 96, 32     # kSwPiece, a unit, units of a piece, kSwHalo, kSwRing
MAX_POINT = 88                                            # kSwMaxPointBytes
JUMP_BYTES = 2 * PIECE + MAX_POINT * 16                   # MODE 1: kWaveBytes - kJumpOff, where kept values go
CHUNK = 32768
RES = 0.5
QF32, LF32, LF64, INT, COPY, XOR32, XOR64 = range(7)      # DevOp::kind (stage1_device.h)
_SIZE = {F.INT8: 1, F.UINT8: 1, F.INT16: 2, F.UINT16: 2, F.INT32: 4, F.UINT32: 4, F.FLOAT32: 4, F.FLOAT64: 8, F.INT64: 8, F.UINT64: 8}

split_chunks, chunk_points, varint_len = PC.split_chunks, PC.chunk_points, PC.varint_len


# ---------------------------------------------------------------------------------------------------------------------
# schemas
# ---------------------------------------------------------------------------------------------------------------------
def plan_of(fields, version, enc):
    """(ops [(kind, size, offset, field index)], adaptive [(bpv, offset, field index)], uses_v5): cldn_hip_plan_create restated"""
    lossy = enc == EncodingOptions.LOSSY
    lead = 0
    if lossy:
        for f in fields:
            if f[2] != F.FLOAT32 or f[3] is None:
                break
            lead += 1
        if lead not in (3, 4):
            lead = 0
    ints = (F.INT16, F.UINT16, F.INT32, F.UINT32, F.INT64, F.UINT64)
    v5 = version >= 5 and lossy and any(f[2] in ints for f in fields[lead:])
    ops, adaptive = [], []
    for i, f in enumerate(fields):
        size = _SIZE[f[2]]
        if enc == EncodingOptions.NONE:
            ops.append((COPY, size, f[1], i))
        elif i < lead:
            ops.append((QF32, 4, f[1], i))
        elif v5 and f[2] in ints:
            adaptive.append((size, f[1], i))
        elif f[2] == F.FLOAT32:
            ops.append((LF32 if lossy and f[3] is not None else (XOR32 if enc == EncodingOptions.LOSSLESS else COPY), 4, f[1], i))
        elif f[2] == F.FLOAT64:
            assert lossy and f[3] is not None or f[3] is not None or version < 4, "a Gorilla op: not this grid's"
            ops.append((LF64 if lossy else XOR64, 8, f[1], i))
        elif f[2] in (F.INT8, F.UINT8):
            ops.append((COPY, 1, f[1], i))
        else:
            ops.append((INT, size, f[1], i))
    return ops, adaptive, v5


class Schema:
    """fields as cases.make_info takes them; route = what decode_route() must say (regular, marker, sections)."""

    def __init__(self, name, fields, step=None, version=5, enc=EncodingOptions.LOSSY, route="stream", marker="none", sections="none"):
        self.name, self.fields, self.version, self.enc = name, fields, version, enc
        self.step = step if step is not None else max(f[1] + _SIZE[f[2]] for f in fields)
        self.ops, self.adaptive, self.v5 = plan_of(fields, version, enc)
        self.route, self.marker, self.sections = route, marker, sections
        self.nops = len(self.ops)
        self.form = [("r", s) if k in (COPY, XOR32, XOR64) else ("v", 5 if k == QF32 else 10) for k, s, _o, _i in self.ops]
        self.var_ops = [o for o, (t, _s) in enumerate(self.form) if t == "v"]
        self.raw_bytes = sum(s for t, s in self.form if t == "r")
        self.max_regular = sum(s for _t, s in self.form)
        self.padded = self.step > sum(_SIZE[f[2]] for f in fields)

    def info(self, n):
        return cases.make_info(self.fields, self.step, n, enc=self.enc, version=self.version)

    def max_len(self, o):
        """the longest token op o admits"""
        k, s = self.ops[o][0], self.ops[o][1]
        return 5 if k == QF32 or (k == INT and s <= 4) else 10

    def wide(self, o):
        k, s = self.ops[o][0], self.ops[o][1]
        return k == LF64 or (k == INT and s == 8)


def _lay(spec, first=0, pad=0):
    """fields from type codes, packed from `first`: q / f = FLOAT32 with a resolution, d = FLOAT64 with one, i = INT32, I = INT64,
    u = UINT16, U = UINT32, b = UINT8, r = FLOAT32 without a resolution, D = FLOAT64 with a resolution (XOR64 under LOSSLESS)"""
    T = {"q": (F.FLOAT32, RES), "f": (F.FLOAT32, RES), "d": (F.FLOAT64, RES), "i": (F.INT32, None), "I": (F.INT64, None),
         "u": (F.UINT16, None), "U": (F.UINT32, None), "b": (F.UINT8, None), "r": (F.FLOAT32, None), "D": (F.FLOAT64, RES)}
    out, off = [], first
    for k, c in enumerate(spec):
        t, res = T[c]
        out.append(("%s%d" % (c, k), off, t, res))
        off += _SIZE[t] + pad
    return out


LOSSLESS, NONE = EncodingOptions.LOSSLESS, EncodingOptions.NONE
SCHEMAS = {s.name: s for s in (
    # stream: n_ops 1..8
    Schema("F1", _lay("f")), Schema("F2", _lay("ff")), Schema("FDF", _lay("fdf")), Schema("XYZ_D", _lay("qqqd")),
    Schema("F5", _lay("fffff")), Schema("XYZ_D_F", _lay("qqqdf")), Schema("F6", _lay("ffffff")), Schema("F7", _lay("fffffff"), step=30),
    Schema("F8", _lay("ffffffff")),
    Schema("I32", _lay("i"), version=4), Schema("I64x8", _lay("IIIIIIII"), version=4), Schema("XYZ_I32_I64", _lay("qqqiI"), version=4, step=27),
    # stream_cols: the float op lists in front of one small UINT16 field
    Schema("F1_U16", _lay("fu"), route="stream_cols", sections="small_general"),
    Schema("F2_U16", _lay("ffu"), route="stream_cols", sections="small_general"),
    Schema("FDF_U16", _lay("fdfu"), route="stream_cols", sections="small_general"),
    Schema("XYZ_D_U16", _lay("qqqdu"), route="stream_cols", sections="small_general"),
    Schema("F5_U16", _lay("fffffu"), route="stream_cols", sections="small_general"),
    Schema("XYZ_D_F_U16", _lay("qqqdfu"), route="stream_cols", sections="small_general"),
    Schema("F6_U16", _lay("ffffffu"), route="stream_cols", sections="small_general"),
    Schema("F7_U16", _lay("fffffffu"), step=33, route="stream_cols", sections="small_general"),
    Schema("F8_U16", _lay("ffffffffu"), route="stream_cols", sections="small_general"),
    # stream_bitmap: automaton32 (7 and 8 states), automaton64 (11 and 16 states; raw sizes 1, 4 and 8)
    Schema("XYZ_R4", _lay("qqqr"), route="stream_bitmap", marker="automaton32"),
    Schema("XYZ_R4_B", _lay("qqqrb"), step=19, route="stream_bitmap", marker="automaton32"),
    Schema("I32_X8_B_X4", _lay("iDbf"), enc=LOSSLESS, route="stream_bitmap", marker="automaton64"),
    Schema("XYZ_3R4_B", _lay("qqqrrrb"), route="stream_bitmap", marker="automaton64"),
    # (15 states, points of up to 78 bytes: the most eight ops with a raw field can have)
    Schema("I64x7_X8", _lay("IIIIIIID"), enc=LOSSLESS, version=4, route="stream_bitmap", marker="automaton64"),
    # form: more than 16 states; maxpt <= 64 and maxpt > 64 (76: the most eight ops with more than 16 states can have -- a seventh
    # varint leaves room for 8 raw bytes, 15 states); the last one has 57 points of 64 value bytes in a piece: not kept
    Schema("XYZ_3R4_2B", _lay("qqqrrrbb"), route="form"),
    Schema("F_D_6R", _lay("fdrrrrrr"), route="form"),
    Schema("I64x6_2X8", _lay("IIIIIIDD"), enc=LOSSLESS, version=4, route="form"),
    Schema("I64_5B_R4_X8", _lay("IbbbbbfD"), enc=LOSSLESS, version=4, route="form"),
    # fixed
    Schema("QUAD", _lay("rrrr"), enc=LOSSLESS, route="fixed"),
    Schema("FIXED_MIXED", _lay("brDrb", first=1), enc=LOSSLESS, step=21, route="fixed"),
    Schema("FIXED_8", _lay("brDrbrDb"), enc=LOSSLESS, route="fixed"),
    # side-by-side sections behind a bitmap-mode stream: the stream kernel in section mode on the DeltaVarint sections
    Schema("XYZ_R4_U16_U32", _lay("qqqruU"), route="stream_bitmap", marker="automaton32", sections="side_by_side"),
    Schema("XYZ_R4_U32", _lay("qqqrU"), route="stream_bitmap", marker="automaton32", sections="side_by_side"),
)}
TWIN = {"F1": "F1_U16", "F2": "F2_U16", "FDF": "FDF_U16", "XYZ_D": "XYZ_D_U16", "F5": "F5_U16", "XYZ_D_F": "XYZ_D_F_U16", "F6": "F6_U16",
        "F7": "F7_U16", "F8": "F8_U16"}
# routes asserted and nothing else: eight ops stay below kSwMaxPointBytes (8 x 10 bytes), so the smallest plan the stream kernel does
# not get has nine ops; all-raw plans of 9 fields likewise (the stream kernel's fixed_F path outside section mode has no plan)
ROUTE_ONLY = {
    "F9": (_lay("fffffffff"), 5, EncodingOptions.LOSSY, "serial"),
    "ALL_RAW_9": (_lay("rrrrrrrrr"), 5, LOSSLESS, "serial"),
    "ALL_RAW_9_NONE": (_lay("bbbbbbbbb"), 5, NONE, "serial"),
}


# ---------------------------------------------------------------------------------------------------------------------
# token codes -> columns
# ---------------------------------------------------------------------------------------------------------------------
def magnitude(L, wide):
    if L <= 1:
        return 0
    if not wide:
        return 1 << (7 * (L - 1) - 1)
    return 1 << 62 if L == 10 else 1 << (7 * L - 2)


def lane_ticks(codes, wide, signs=None):
    """(q int64 [n], nan mask): running sums whose tokens have the codes. A narrow lane's token of 6 bytes or more (Float_Lossy<float>
    only) jumps to exactly 1.5 m(L) -- float32 could not hold the small classes next to it -- and the next one of its class back to 0."""
    ln = np.asarray(codes, dtype=np.int64)
    n = len(ln)
    mag = np.array([magnitude(int(L), wide) for L in ln], dtype=np.int64)
    sgn = np.ones(n, dtype=np.int64)
    for k in range(2, 11):
        idx = np.nonzero(ln == k)[0]
        sgn[idx] = np.where(np.arange(len(idx)) & 1, -1, 1)
    if signs is not None:
        sgn = np.where(np.asarray(signs) != 0, np.asarray(signs), sgn)
    nan = ln == 0
    if not wide and ln.max(initial=0) >= 6:
        q, cur = np.empty(n, dtype=np.int64), 0
        for i in range(n):
            L = int(ln[i])
            if L == 0:
                cur = 0
            elif L >= 6:
                cur = 0 if abs(cur) >= (1 << 33) else 3 * (int(mag[i]) >> 1)
            else:
                assert L == 1 or abs(cur) < (1 << 33), "a short token while a long one is up"
                cur += int(mag[i]) * int(sgn[i])
            q[i] = cur
        return q, nan
    with np.errstate(over="ignore"):
        cs = np.cumsum(mag * sgn)          # (int64 wrap-around is what a 64-bit field does)
        last = np.maximum.accumulate(np.where(nan, np.arange(n), -1))
        q = cs - np.where(last >= 0, cs[last.clip(0)], 0)
    return q, nan


def column(codes, kind, size, signs=None):
    """the field's column whose tokens have the codes"""
    wide = kind == LF64 or (kind == INT and size == 8)
    q, nan = lane_ticks(codes, wide, signs)
    if kind == INT:
        assert not nan.any(), "a marker on an integer op is malformed"
        if size == 8:
            return q
        assert np.abs(q).max(initial=0) < (1 << 31)
        return q.astype(np.int32)
    dt = np.float64 if kind == LF64 else np.float32
    x = (q.astype(np.float64) * RES).astype(dt)
    back = np.round(x.astype(np.float64) / RES)
    assert np.array_equal(back, q.astype(np.float64)) and np.abs(q).max(initial=0) < (1 << 63), "ticks not exactly representable"
    if kind != LF64:
        assert np.array_equal(x.astype(np.float64), q.astype(np.float64) * RES)
        assert kind != QF32 or np.abs(q).max(initial=0) < (1 << 30)
    else:
        # a double holds 53 bits: the span of the set bits must fit
        assert all(int(v) == int(np.float64(int(v))) for v in q[:: max(1, len(q) // 4096)])
    x[nan] = np.nan
    return x


def raw_column(kind_size, ftype, n, pattern):
    """chosen bytes for a raw field: pattern(i, b) -> byte b of point i's STREAM token (XOR fields: the stream holds prev ^ cur, so the
    column is the running XOR of the pattern)"""
    kind, size = kind_size
    i = np.arange(n, dtype=np.int64)
    tok = np.zeros(n, dtype=np.uint64)
    for b in range(size):
        tok |= (np.asarray(pattern(i, b), dtype=np.uint64) & np.uint64(0xFF)) << np.uint64(8 * b)
    if kind in (XOR32, XOR64):
        tok = np.bitwise_xor.accumulate(tok)
    return tok.astype("<u%d" % size).view(cases._NP[ftype])


def bytes_any(i, b):
    return (i * 37 + b * 101 + (i >> 3)) & 0xFF


def bytes_edges(i, b):
    """0x00, 0x7f, 0x80 and 0xff runs, eight points each"""
    return np.array([0x00, 0x7F, 0x80, 0xFF], dtype=np.int64)[(i >> 3) & 3]


def bytes_xor_returns(i, b):
    """the running XOR returns to 0 every second point"""
    return ((i >> 1) * 29 + b * 7 + 1) & 0xFF


# ---------------------------------------------------------------------------------------------------------------------
# whole points of chosen size
# ---------------------------------------------------------------------------------------------------------------------
def fill_points(nbytes, schema, long_ok=5):
    """[codes of a point] * k: whole points (varint tokens of 1..5 bytes, mostly 2) whose regular-stream bytes sum to nbytes"""
    nv, R = len(schema.var_ops), schema.raw_bytes
    if nbytes == 0:
        return []
    lo, hi = R + nv, R + long_ok * nv
    k = max(1, nbytes // (R + 2 * nv) if nv else nbytes // R)
    while k * hi < nbytes:
        k += 1
    while k * lo > nbytes:
        k -= 1
    assert k >= 1 and k * lo <= nbytes <= k * hi, (nbytes, schema.name)
    t, e = k * nv, nbytes - k * lo
    ln = [1 + e // t + (1 if i < e % t else 0) for i in range(t)] if t else []
    if t and t % 7:
        ln = [ln[(i * 7) % t] for i in range(t)]
    return [ln[j * nv:(j + 1) * nv] for j in range(k)]


def point_bytes(schema, pt):
    return schema.raw_bytes + sum(max(1, c) for c in pt)


def compose(a0, schema, items, total=None, more=0, long_ok=5):
    """[codes of a point]. items in stream order: ("point", V, codes) = a point with these codes begins at v = V; ("run", [points]).
    Whole filler points go in between. Behind the last item about `more` bytes of filler follow, or filler up to a payload of `total`."""
    pts, off = [], 0
    for it in items:
        if it[0] == "run":
            pts += [list(p) for p in it[1]]
            off += sum(point_bytes(schema, p) for p in it[1])
            continue
        _p, V, codes = it
        gap = V - a0 - off
        assert gap >= 0, (it, off)
        pts += fill_points(gap, schema, long_ok) + [list(codes)]
        off = V - a0 + point_bytes(schema, codes)
    if total is not None:
        pts += fill_points(total - off, schema, long_ok)
    elif more:      # (about `more` bytes: whole points of 2-byte tokens)
        pts += [[2] * len(schema.var_ops)] * max(1, more // point_bytes(schema, [2] * len(schema.var_ops)))
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# the piece model
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    """Of one chunk: payload, a0, the point's form ([("v", max) | ("r", size)]), n points. ends / lens: the regular stream's tokens
    (payload offset of the last byte, bytes; raw fields are tokens of their size); reg_end. Per piece p: T0[p] token ends in front of
    it and cnt[p] in it, as the kernel counts them with MSB ends: every payload byte with a clear MSB, section bytes included (bitmap
    and form rows: the regular tokens only -- what the marker writes behind the regular stream is not this model's). stop[p]: the
    regular stream ended in front of the piece. start[q] / owner[q] / row[q] / lane[q]: where point q begins, the piece that owns it
    (MODE 0 rule; owner_form: MODE 1 rule) and its place among the piece's points. k0s: {(n_ops, k0)} over the units that hold a token
    end of pieces that are not stopped. entry[p] (MODE 1): offset in the piece of the first point that begins in it, None = none.
    keep[p] (MODE 1): the first walk's values fit where the jump table was."""

    def __init__(self, payload, a0, schema, n):
        p = np.asarray(payload, dtype=np.uint8)
        form, nops = schema.form, schema.nops
        self.payload, self.a0, self.schema, self.n, self.nops = p, a0, schema, n, nops
        target = n * nops
        self.msb_mode = all(t == "v" for t, _s in form)
        if self.msb_mode:
            all_ends = np.nonzero(p < 0x80)[0]
            assert len(all_ends) >= target
            self.ends = all_ends[:target]
        else:
            clear = np.nonzero(p < 0x80)[0]
            ends, off = np.empty(target, dtype=np.int64), 0
            sizes = [s if t == "r" else 0 for t, s in form]
            for q in range(n):
                for o, s in enumerate(sizes):
                    if s:
                        off += s
                    else:
                        off = int(clear[np.searchsorted(clear, off)]) + 1
                    ends[q * nops + o] = off - 1
            assert off <= len(p)
            self.ends = all_ends = ends
        self.lens = np.diff(self.ends, prepend=-1)
        self.reg_end = int(self.ends[-1]) + 1 if target else 0
        self.vend = a0 + len(p)
        self.n_pieces = (self.vend + PIECE - 1) // PIECE if len(p) else 0
        edges = np.arange(self.n_pieces + 1) * PIECE
        self.T0 = np.searchsorted(all_ends + a0, edges[:-1])
        self.cnt = np.searchsorted(all_ends + a0, edges[1:]) - self.T0
        self.stop = self.T0 >= target
        self.stop[0:1] = False
        v = self.ends + a0
        self.start = np.concatenate([[0], self.ends[nops - 1::nops][:-1] + 1]) if n else np.zeros(0, np.int64)
        self.owner = np.concatenate([[0], v[nops - 1::nops][:-1] // PIECE]) if n else np.zeros(0, np.int64)
        self.owner_form = (self.start + a0) // PIECE
        first = np.searchsorted(self.owner, np.arange(self.n_pieces))
        self.owned = np.searchsorted(self.owner, np.arange(self.n_pieces), side="right") - first
        j = np.arange(n) - first[self.owner] if n else np.zeros(0, np.int64)
        self.row, self.lane = j // 64, j % 64
        self.point_len = np.diff(np.concatenate([self.start, [self.reg_end]])) if n else np.zeros(0, np.int64)
        # k0 of every unit that holds a token end of a piece at work: the tokens its first end still has to skip
        idx = np.arange(target)
        unit = v // UNIT
        first_in_unit = np.concatenate([[True], unit[1:] != unit[:-1]]) if target else np.zeros(0, bool)
        self.k0_of_unit = {int(u): int(nops - 1 - i % nops) for u, i in zip(unit[first_in_unit], idx[first_in_unit])}
        self.k0s = {(nops, k) for k in self.k0_of_unit.values()}
        # MODE 1
        f1 = np.searchsorted(self.owner_form, np.arange(self.n_pieces))
        self.owned_form = np.searchsorted(self.owner_form, np.arange(self.n_pieces), side="right") - f1
        self.entry = [int(self.start[f] + a0 - pc * PIECE) if k else None for pc, (f, k) in enumerate(zip(f1, self.owned_form))]
        vtot = sum(4 if (kd == QF32 or (kd == INT and sz <= 4)) else 8 for kd, sz, _o, _i in schema.ops)
        npad = (self.owned_form + 1) & ~1
        self.keep = (((npad * vtot + 7) & ~7) + (self.owned_form + 63) // 64 * nops * 8 <= JUMP_BYTES) & (self.owned_form > 0)
        # the unit in which the regular stream ends, and the first piece that holds nothing of it
        self.target_unit = ((self.reg_end - 1 + a0) % PIECE) // UNIT if target else None

    def token_v(self):
        return self.ends + self.a0

    def candidate_exit(self, piece, offset):
        """MODE 1: where a candidate that follows the point's form from byte `offset` of `piece` enters the next piece (its offset
        there); None if it meets a varint without an end in 10 bytes or leaves the payload -- a dead candidate"""
        x, p = piece * PIECE + offset - self.a0, self.payload
        while x + self.a0 < (piece + 1) * PIECE:
            for t, size in self.schema.form:
                if t == "r":
                    x += size
                else:
                    e = np.nonzero(p[x:x + 10] < 0x80)[0]
                    if not len(e):
                        return None
                    x += int(e[0]) + 1
            if x > len(p):
                return None
        return x + self.a0 - (piece + 1) * PIECE

    def code_lens(self):
        """[n, n_ops] token bytes"""
        return self.lens.reshape(self.n, self.nops)

    def place(self):
        """(owner, row, lane) of every point by the rule of the schema's route (MODE 1 for `form`)"""
        if self.schema.route != "form":
            return self.owner, self.row, self.lane
        first = np.searchsorted(self.owner_form, np.arange(self.n_pieces))
        j = np.arange(self.n) - first[self.owner_form]
        return self.owner_form, j // 64, j % 64

    def rows_with_long(self):
        """{(piece, row): sorted lanes whose point has a token of more than 4 bytes}, every (piece, row) present"""
        out = {}
        long_pt = (self.code_lens()[:, self.schema.var_ops] > 4).any(axis=1) if self.n else np.zeros(0, bool)
        owner, row, lane = self.place()
        for q in range(self.n):
            out.setdefault((int(owner[q]), int(row[q])), [])
            if long_pt[q]:
                out[(int(owner[q]), int(row[q]))].append(int(lane[q]))
        return out

    def markers(self):
        """[n, n_ops] bool: the token is the one byte 0x00 of a float op"""
        first = self.payload[self.ends - self.lens + 1] if len(self.ends) else np.zeros(0, np.uint8)
        mk = ((self.lens == 1) & (first == 0)).reshape(self.n, self.nops)
        floats = np.array([k in (QF32, LF32, LF64) for k, _s, _o, _i in self.schema.ops])
        return mk & floats[None, :]


def serial_model(payload, a0, schema, n):
    """The same facts by a walk over the bytes, one at a time: (ends, reg_end, T0, cnt, owner, row, lane, k0 per unit, entry, owner_form,
    points that begin in each piece, the v of the last regular token end)"""
    p = bytes(np.asarray(payload, dtype=np.uint8).tobytes())
    nops, form = schema.nops, schema.form
    msb = all(t == "v" for t, _s in form)
    vend = a0 + len(p)
    n_pieces = (vend + PIECE - 1) // PIECE if p else 0
    T0, cnt = [0] * n_pieces, [0] * n_pieces
    ends, owner, row, lane, k0, owner_form = [], [0] if n else [], [0] if n else [], [0] if n else [], {}, [0 + a0 // PIECE] if n else []
    entry = [None] * n_pieces
    if n:
        entry[a0 // PIECE] = a0 % PIECE
    in_piece = {0: 1}
    seen, o, left = 0, 0, form[0][1] if form[0][0] == "r" else 0
    for off, byte in enumerate(p):
        v = off + a0
        if seen < n * nops:
            if form[o][0] == "r":
                left -= 1
                is_end = left == 0
            else:
                is_end = not byte & 0x80
        else:
            is_end = msb and not byte & 0x80
        if not is_end:
            continue
        pc = v // PIECE
        cnt[pc] += 1
        for later in range(pc + 1, n_pieces):
            T0[later] += 1
        if seen >= n * nops:
            continue
        ends.append(off)
        if v // UNIT not in k0:
            k0[v // UNIT] = nops - 1 - seen % nops
        seen += 1
        o = seen % nops
        left = form[o][1] if form[o][0] == "r" else 0
        if o == 0 and seen < n * nops:          # the byte behind begins a point
            owner.append(pc)
            row.append(in_piece.get(pc, 0) // 64)
            lane.append(in_piece.get(pc, 0) % 64)
            in_piece[pc] = in_piece.get(pc, 0) + 1
            pf = (v + 1) // PIECE
            owner_form.append(pf)
            if entry[pf] is None:
                entry[pf] = (v + 1) % PIECE
    begin = [0] * n_pieces
    for pf in owner_form:
        begin[pf] += 1
    return ends, (ends[-1] + 1 if ends else 0), T0, cnt, owner, row, lane, k0, entry, owner_form, begin, (ends[-1] + a0 if ends else None)


def section_models(m):
    """One Model per integer field of the chunk whose Model is m: its DeltaVarint section (mode byte 0) as a stream of n tokens of one
    integer op at its own a0 -- the bytes behind the mode byte, as the stream kernel's section mode gets them. None if a section has
    another mode."""
    p, pos, out = m.payload, m.reg_end, []
    for _a in m.schema.adaptive:
        if pos >= len(p) or p[pos] != 0:
            return None
        pos += 1
        ends = np.nonzero(p[pos:] < 0x80)[0][:m.n]
        if len(ends) < m.n:
            return None
        end = pos + int(ends[-1]) + 1
        out.append(Model(p[pos:end], (m.a0 + pos) % 16, SCHEMAS["I32"], m.n))
        pos = end
    return out if pos == len(p) else None


def models(streams, ns, a0, schema):
    """One Model per chunk of a batch whose streams lie back to back, the first payload at residue a0."""
    out, base = [], a0 - 4
    for stream, n in zip(streams, ns):
        for (off, payload), k in zip(split_chunks(stream), chunk_points(n)):
            out.append(Model(payload, (base + off) % 16, schema, k))
        base += len(stream)
    return out


# ---------------------------------------------------------------------------------------------------------------------
class Row:
    """build(a0) -> [(points, signs)] per cloud: points = [codes of a point's varint ops], signs = None or the same shape (+-1, 0 =
    the rule). raw = the byte pattern of the raw fields. pred(M, a0), M = one Model per chunk. a0s: the residues the GPU test runs
    the row at."""

    def __init__(self, name, family, schema, build, pred, a0s=(4,), raw=bytes_any, ints=None, sect=None, modes=None):
        self.name, self.family, self.schema, self.build, self.pred, self.a0s = name, family, SCHEMAS[schema], build, pred, tuple(a0s)
        self.raw, self.ints = raw, ints
        self.sect, self.modes = sect, modes      # sect(a0, n) -> {k: column of integer field k}; modes: the section modes, forced
        self.base = None

    @property
    def sections(self):
        return bool(self.schema.adaptive)

    def info(self, n):
        return self.schema.info(n)

    def clouds(self, a0):
        S, out = self.schema, []
        for pts, signs in self.build(a0):
            n = len(pts)
            c = np.asarray(pts, dtype=np.int64).reshape(n, len(S.var_ops))
            sg = None if signs is None else np.asarray(signs, dtype=np.int64).reshape(n, len(S.var_ops))
            cols = {}
            for k, o in enumerate(S.var_ops):
                kind, size, _off, fi = S.ops[o]
                assert c[:, k].max(initial=1) <= S.max_len(o)
                cols[S.fields[fi][0]] = column(c[:, k], kind, size, None if sg is None else sg[:, k])
            for o, (kind, size, _off, fi) in enumerate(S.ops):
                if kind in (COPY, XOR32, XOR64):
                    cols[S.fields[fi][0]] = raw_column((kind, size), S.fields[fi][2], n, lambda i, b, o=o: self.raw(i + o, b))
            i = np.arange(n, dtype=np.int64)
            for k, (_bpv, _off, fi) in enumerate(S.adaptive):
                f = S.fields[fi]
                chosen = self.sect(a0, n) if self.sect else {}
                v = chosen[k] if k in chosen else (self.ints(k, i) if self.ints else (i * (3 + 2 * k) // 5) % (3 + k) * 257 + k)
                cols[f[0]] = np.asarray(v).astype(cases._NP[f[2]])
            out.append((n, cases.pack(self.info(n), cols, n)))
        return out

    def streams(self, oracle, a0):
        cl = self.clouds(a0)
        if self.modes is not None:
            st = [oracle.encode_stage1_continued(self.info(n), c, self.modes) for n, c in cl]
        else:
            st = [oracle.encode_stage1(self.info(n), c) for n, c in cl]
        return st, [n for n, _c in cl], [c for _n, c in cl]

    def models(self, streams, ns, a0):
        return models(streams, ns, a0, self.schema)


def pinned(row):
    """The row's regular stream, byte for byte, in front of one small UINT16 field (a Palette section): the `stream_cols` twin, where
    sec_done == 2 shows that the stream kernel kept the chunk. The twin's predicate: a section follows (that its regular stream is the
    base row's payload is carries_the_base_tokens; where the payload ends is the base row's own fact)."""
    twin = Row(row.name, row.family, TWIN[row.schema.name], row.build, lambda M, a0: all(m.reg_end < len(m.payload) for m in M), row.a0s, row.raw)
    twin.base = row
    return twin


def carries_the_base_tokens(M, base_M):
    return len(M) == len(base_M) and all(np.array_equal(m.payload[:m.reg_end], b.payload[:b.reg_end]) and m.n == b.n and
                                         b.reg_end == len(b.payload) for m, b in zip(M, base_M))


# ---- predicates
def all_of(*preds):
    return lambda M, a0: all(p(M, a0) for p in preds)


def point_at(V, lens=None, chunk=0):
    """a point begins at v = V (and its tokens have these lengths)"""
    def pred(M, a0):
        m = M[chunk]
        q = np.nonzero(m.start + m.a0 == V)[0]
        return len(q) == 1 and (lens is None or m.code_lens()[q[0]].tolist() == list(lens))
    return pred


def token_ends_at(V, length=None, chunk=0):
    def pred(M, a0):
        m = M[chunk]
        i = np.nonzero(m.token_v() == V)[0]
        return len(i) == 1 and (length is None or m.lens[i[0]] == length)
    return pred


def pieces(k, chunk=0):
    return lambda M, a0: M[chunk].n_pieces == k


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
STREAM = ("F1", "F2", "FDF", "XYZ_D", "F5", "XYZ_D_F", "F6", "F7", "F8")       # n_ops 1..8 (two of 5): rows with a stream_cols twin
STREAM_V4 = ("I32", "I64x8", "XYZ_I32_I64")                                     # integer ops: the version-4 wire has no sections
BITMAP = ("XYZ_R4", "XYZ_R4_B", "I32_X8_B_X4", "XYZ_3R4_B", "I64x7_X8")
FORM = ("XYZ_3R4_2B", "F_D_6R", "I64x6_2X8", "I64_5B_R4_X8")
FIXED = ("QUAD", "FIXED_MIXED", "FIXED_8")
SECTION = ("XYZ_R4_U16_U32", "XYZ_R4_U32")


def _one(fn):
    def build(a0):
        r = fn(a0)
        return [r if isinstance(r, tuple) else (r, None)]
    return build


def _ones(S):
    return [1] * len(S.var_ops)


def _with(S, k, L):
    pt = _ones(S)
    pt[k] = L
    return pt


def _length_rows(T):
    # A: every length every varint op admits, in every op position, up and down; f32 lanes take 6..10 one class at a time
    for name in STREAM + STREAM_V4 + BITMAP + FORM:
        S = SCHEMAS[name]

        def fn(a0, S=S):
            pts = []
            for k, o in enumerate(S.var_ops):
                for L in range(1, S.max_len(o) + 1):
                    pts += [_with(S, k, L), _ones(S), _with(S, k, L), _ones(S)]
            return pts

        def pred(M, a0, S=S):
            cl = M[0].code_lens()
            return all(int((cl[:, o] == L).sum()) >= 2 for o in S.var_ops for L in range(1, S.max_len(o) + 1))
        T.append(Row("lengths_every_op_" + name, "A", name, _one(fn), pred))

    # A: a row of 64 points with exactly one token of more than 4 bytes, in lane 0 / lane 63, and rows with none (sw_token32 against
    # sw_token); lengths 8, 9 and 10 in one row of points
    for name in ("F2", "XYZ_D", "F8", "I64x8", "XYZ_I32_I64", "XYZ_R4", "XYZ_3R4_2B"):
        S = SCHEMAS[name]
        for lane in (0, 63):
            if lane * point_bytes(S, _ones(S)) >= PIECE:      # (a piece owns fewer than 64 such points)
                continue

            def fn(a0, S=S, lane=lane):
                # points of 1-byte tokens: point q begins at v = a0 + q B. The first point piece 1 owns, + lane
                k = len(S.var_ops) - 1
                L = S.max_len(S.var_ops[k])
                B = point_bytes(S, _ones(S))
                q1 = (PIECE - a0 + B - 1) // B + (0 if S.route == "form" else 1)
                while (a0 + q1 * B - (0 if S.route == "form" else 1)) // PIECE < 1:
                    q1 += 1
                while (a0 + (q1 - 1) * B - (0 if S.route == "form" else 1)) // PIECE >= 1:
                    q1 -= 1
                pts = [_ones(S) for _ in range(q1 + 64 + 3 * PIECE // B)]
                pts[q1 + lane], pts[-2] = _with(S, k, L), _with(S, k, L)
                return pts

            def pred(M, a0, lane=lane):
                rows = M[0].rows_with_long()
                return rows.get((1, 0)) == [lane] and [] in rows.values() and sum(len(v) for v in rows.values()) == 2
            T.append(Row("one_long_token_in_lane_%d_%s" % (lane, name), "A", name, _one(fn), pred))
    for name in ("F2", "XYZ_D", "I64x8", "I64x7_X8", "I64x6_2X8"):
        S = SCHEMAS[name]
        wide = [k for k, o in enumerate(S.var_ops) if S.max_len(o) == 10]

        def fn(a0, S=S, wide=wide):
            pts = []
            for L in (8, 9, 10):
                for k in wide:
                    pts += [_with(S, k, L), _with(S, k, L)]
            return pts + [_ones(S)] * 3
        T.append(Row("lengths_8_9_10_" + name, "A", name, _one(fn),
                     lambda M, a0, S=S, wide=wide: all(int((M[0].code_lens()[:, S.var_ops[k]] == L).sum()) == 2 for k in wide for L in (8, 9, 10))))

    # A: a 64-bit running value that wraps: +2^62 four times, in every INT64 op, across a row boundary
    def fn(a0):
        S = SCHEMAS["I64x8"]
        pts = [_ones(S) for _ in range(62)] + [[10] * 8 for _ in range(8)] + [_ones(S)] * 3
        signs = [[0] * 8 for _ in range(62)] + [[1] * 8 for _ in range(8)] + [[0] * 8] * 3
        return pts, signs
    T.append(Row("wrap_64_bit_running_value", "A", "I64x8", _one(fn),
                 lambda M, a0: int((M[0].code_lens() == 10).sum()) == 64 and M[0].n == 73))


def _edge_rows(T, names, family, a0s):
    # B / F: piece edges. A point (the longest the fill makes: every varint 4 bytes) that ends at byte 1023, begins at 1024, straddles
    # 1024 with 1 and with all but 1 of its bytes in front; the last token of a point ending at 1023 / first token beginning at 1024
    for name in names:
        S = SCHEMAS[name]
        big = [4] * len(S.var_ops)
        size = point_bytes(S, big)
        for what, first in (("ends_at_1023", PIECE - size), ("begins_at_1024", PIECE), ("straddles_1_byte_in_front", PIECE - 1),
                            ("straddles_1_byte_behind", PIECE - size + 1)):
            def fn(a0, S=S, first=first, big=big):
                return compose(a0, S, [("point", first, big), ("point", first + PIECE, big)], more=300)
            T.append(Row("point_%s_%s" % (what, name), family, name, _one(fn),
                         all_of(point_at(first, None), point_at(first + PIECE, None), lambda M, a0, size=size, first=first:
                                M[0].point_len[np.nonzero(M[0].start + M[0].a0 == first)[0][0]] == size), a0s=a0s))


def _halo_rows(T):
    # B / F / G: the point of greatest length beginning at byte 1023 (halo reach; E[3] and the clamp of pos): every op's longest
    # token, up in this point and down in the next. Bitmap schemas at all 16 a0. MODE 1: the next piece is entered at the point's
    # length - 1 (I64x6_2X8: 75, the second candidate set).
    for name in ("F8", "I64x8", "XYZ_D_F", "F2") + BITMAP + FORM:
        S = SCHEMAS[name]

        def fn(a0, S=S):
            longest = [S.max_len(o) for o in S.var_ops]
            return compose(a0, S, [("point", PIECE - 1, longest), ("run", [longest])], more=200)

        def pred(M, a0, S=S):
            m = M[0]
            q = np.nonzero(m.start + m.a0 == PIECE - 1)[0]
            size = point_bytes(S, [S.max_len(o) for o in S.var_ops])
            return len(q) == 1 and m.point_len[q[0]] == size and m.owner[q[0]] == 0 and m.entry[1] == size - 1
        T.append(Row("longest_point_begins_at_1023_" + name, "F" if name in BITMAP else ("G" if name in FORM else "B"), name, _one(fn), pred,
                     a0s=tuple(range(16)) if name in BITMAP + FORM else (4,)))


def _piece_count_rows(T):
    # B: a chunk of exactly 1, 2, 32, 33 and 65 pieces (ring wrap); payloads that end on a unit's last byte and on its first
    for name in ("F2", "XYZ_D", "F8", "XYZ_R4", "I64x7_X8", "XYZ_3R4_2B", "I64x6_2X8"):
        S = SCHEMAS[name]
        for k in (1, 2, 32, 33, 65):
            for tail, what in ((0, "unit_last_byte"), (1, "unit_first_byte")):
                if tail and k not in (1, 33):
                    continue

                def fn(a0, S=S, k=k, tail=tail):
                    return compose(a0, S, [], total=(k - 1) * PIECE + 16 * 20 + tail - a0)
                T.append(Row("pieces_%d_ends_on_%s_%s" % (k, what, name), "F" if name in BITMAP else ("G" if name in FORM else "B"), name, _one(fn),
                             all_of(pieces(k), lambda M, a0, tail=tail: M[0].vend % 16 == tail and M[0].reg_end == len(M[0].payload)),
                             a0s=(4, 13) if name in BITMAP + FORM else (4,)))


def _count_rows(T):
    # C: 1-byte tokens: up to 1024 points per piece, every k0; n = 1, 63, 64, 65; a full chunk; a second chunk
    for name in STREAM + ("I32", "I64x8"):
        S = SCHEMAS[name]
        n_small = (4 * PIECE) // S.nops + 7

        def fn(a0, S=S, n=n_small):      # two pieces of 1-byte tokens; behind them every 17th token has 2 bytes, so every k0 comes up
            flat = [1 if g < 2 * PIECE or g % 17 else 2 for g in range(n * S.nops)]
            return [flat[q * S.nops:(q + 1) * S.nops] for q in range(n)]
        T.append(Row("one_byte_tokens_" + name, "C", name, _one(fn),
                     lambda M, a0, S=S: M[0].lens[:2000].max() == 1 and M[0].n_pieces >= 4 and int(M[0].owned.max()) >= (PIECE - 1) // S.nops and
                     M[0].k0s == {(S.nops, k) for k in range(S.nops)}))
    for name in ("FDF", "F5", "F6", "F7", "F8"):
        S = SCHEMAS[name]
        T.append(Row("full_chunk_one_byte_tokens_" + name, "C", name, _one(lambda a0, S=S: [_ones(S)] * CHUNK),
                     lambda M, a0, S=S: M[0].n == CHUNK and M[0].lens.max() == 1 and int(M[0].T0.max()) > CHUNK * S.nops - PIECE - 16))
    for name in ("F2", "XYZ_D_F", "I64x8"):
        S = SCHEMAS[name]
        for n in (1, 63, 64, 65):
            def fn(a0, S=S, n=n):
                return [[1 + (q * 3 + o) % 3 for o in range(len(S.var_ops))] for q in range(n)]
            T.append(Row("n_%d_%s" % (n, name), "C", name, _one(fn), lambda M, a0, n=n: M[0].n == n and len(M) == 1))
    for name in ("F2", "XYZ_D"):
        S = SCHEMAS[name]
        for n in (CHUNK - 1, CHUNK, CHUNK + 700):
            def fn(a0, S=S, n=n):
                return [[1 + ((q * 5 + o + q // 97) % 12 in (3, 7)) + 2 * ((q * 5 + o) % 12 == 6) for o in range(len(S.var_ops))] for q in range(n)]
            T.append(Row("n_%d_%s" % (n, name), "C", name, _one(fn),
                         lambda M, a0, n=n: sum(m.n for m in M) == n and len(M) == (2 if n > CHUNK else 1) and M[0].n_pieces > 2 * RING))


def _marker_rows(T):
    # D: on a narrow op (XYZ_D op 0: a FloatN lane, 32-bit sums) and on 64-bit ops (Float_Lossy<float / double> keep 64-bit sums).
    # The marker's op climbs 64 ticks with every point (2-byte tokens, always up), so its running value is never 0 where a marker
    # resets it and every carry into a piece is another value: a reset that is dropped, or taken one lane early, changes bytes.
    for name, k in (("XYZ_D", 0), ("XYZ_D", 3), ("F2", 1), ("XYZ_D_F", 4)):
        S = SCHEMAS[name]
        nv = len(S.var_ops)
        tag = "_%s_op%d" % (name, k)
        body = _with(S, k, 2)
        up = [1 if o == k else 0 for o in range(nv)]

        def cloud(n, marked, S=S, k=k, body=body, up=up):
            """n points; marked(q, v, prev) -> point q, which begins at v (the point in front at prev), carries the marker"""
            def build(a0):
                out, at, prev = [], a0, -1
                for q in range(n):
                    pt = list(body)
                    if marked(q, at, prev):
                        pt[k] = 0
                    out.append(pt)
                    prev, at = at, at + point_bytes(S, pt)
                return out, [list(up)] * n
            return build

        def pred_marks(marks, S=S, k=k):
            def pred(M, a0):
                m = M[0]
                mk = m.markers()
                return sorted(np.nonzero(mk[:, S.var_ops[k]])[0].tolist()) == sorted(marks) and int(mk.sum()) == len(marks) and m.owned[0] == m.n
            return pred
        # (piece 0 owns every point: point q is lane q % 64 of row q // 64)
        for what, marks, n in (("lane_0", [64], 130), ("lane_63", [63], 130), ("lanes_0_and_63", [64, 127], 130), ("alone_in_a_row_of_one", [128], 129)):
            T.append(Row("nan_" + what + tag, "D", name, _one(cloud(n, lambda q, v, prev, marks=marks: q in marks)),
                         all_of(pred_marks(marks), lambda M, a0, n=n: M[0].n == n)))

        # NaN in every point piece 1 owns; pieces 0 and 2 have none: the carry into piece 2 starts behind piece 1's last marker
        def pred(M, a0, S=S, k=k):
            m = M[0]
            mk = m.markers()[:, S.var_ops[k]]
            return m.n_pieces >= 4 and mk[m.owner == 1].all() and not mk[m.owner != 1].any() and m.owned[1] > 64
        T.append(Row("nan_in_every_point_of_a_piece" + tag, "D", name,
                     _one(cloud(4 * PIECE // point_bytes(S, body), lambda q, v, prev: q > 0 and PIECE <= v - 1 < 2 * PIECE)), pred))

        # one marker in piece 1 and one in piece 3, values behind each, marker-free pieces 2 and 4 (aggf_l: a piece with a marker
        # drops the carry of the pieces in front, the marker-free piece behind it adds its own sum to that piece's)
        def marked(q, v, prev):
            return any(prev < pc * PIECE + 300 <= v for pc in (1, 3))

        def pred(M, a0, S=S, k=k):
            m = M[0]
            mk = m.markers()[:, S.var_ops[k]]
            return sorted(set(m.owner[mk].tolist())) == [1, 3] and int(mk.sum()) == 2 and m.n_pieces >= 5 and \
                bool((m.owner[np.nonzero(mk)[0] + 40] == [1, 3]).all())
        T.append(Row("nan_then_carry_into_marker_free_pieces" + tag, "D", name, _one(cloud(5 * PIECE // point_bytes(S, body) + 20, marked)), pred))


def _regend_rows(T):
    # E: the end of the regular stream: sections behind it whose bytes all have clear MSBs (a Palette of small values), `target`
    # reached in a piece's last unit and in its first, and pieces that hold only section bytes (`stop`)
    for name in ("F2_U16", "XYZ_D_U16", "F8_U16"):
        S = SCHEMAS[name]
        for what, last_v in (("last_unit", 2 * PIECE - 3), ("first_unit", 2 * PIECE + 5)):
            def fn(a0, S=S, last_v=last_v):
                return compose(a0, S, [], total=last_v + 1 - a0)

            def pred(M, a0, S=S, last_v=last_v, what=what):
                m = M[0]
                behind = m.payload[m.reg_end:]
                return m.reg_end - 1 + a0 == last_v and m.target_unit == (63 if what == "last_unit" else 0) and len(behind) > 8 and \
                    bool((behind < 0x80).all())
            T.append(Row("regular_end_in_the_%s_%s" % (what, name), "E", name, _one(fn), pred, ints=lambda k, i: (i % 8 == 1) | (i % 8 == 2)))

        # sections of more than a piece behind the regular stream: every value its own (no Palette), clear MSBs
        def fn(a0, S=S):
            return compose(a0, S, [], total=PIECE - 60 - a0)

        def pred(M, a0):
            m = M[0]
            return bool(m.stop[1:].all()) and m.n_pieces >= 2 and m.reg_end + a0 == PIECE - 60
        T.append(Row("pieces_of_section_bytes_only_" + name, "E", name, _one(fn), pred, ints=lambda k, i: (i * i * 7 + i * 3) % 127 * 129 % 16384))


def _raw_rows(T):
    # F / G: raw fields of 0x00 / 0x7f / 0x80 / 0xff runs (bytes that read as token ends and as continuations at every offset of the
    # point), both parities of the second chunk's src_off
    for name in BITMAP + FORM:
        S = SCHEMAS[name]
        n = 3 * PIECE // point_bytes(S, [2] * len(S.var_ops)) + 30
        T.append(Row("raw_runs_of_00_7f_80_ff_" + name, "F" if name in BITMAP else "G", name,
                     _one(lambda a0, S=S, n=n: [[1 + (q + o) % 3 for o in range(len(S.var_ops))] for q in range(n)]),
                     lambda M, a0, S=S: M[0].n_pieces >= 2 and {0x00, 0x7F, 0x80, 0xFF} <= set(
                         M[0].payload[M[0].ends[[o for o, (t, _s) in enumerate(S.form) if t == "r"][0]::S.nops]].tolist()),
                     raw=bytes_edges, a0s=(4, 11)))
    for name in ("XYZ_R4", "XYZ_3R4_B", "XYZ_3R4_2B"):
        S = SCHEMAS[name]
        for parity in (0, 1):
            def fn(a0, S=S, parity=parity):
                pts = [[1 + (q * 5 + o) % 4 for o in range(len(S.var_ops))] for q in range(CHUNK + 300)]
                size = sum(point_bytes(S, p) for p in pts[:CHUNK])
                if (size + 8) % 2 != parity:       # the second payload's offset in the batch: the first chunk's size + two size words
                    pts[0][0] += 1
                return pts
            T.append(Row("second_chunk_src_off_parity_%d_%s" % (parity, name), "F" if name in BITMAP else "G", name, _one(fn),
                         lambda M, a0, parity=parity: len(M) == 2 and (len(M[0].payload) + 8) % 2 == parity))


def _form_rows(T):
    # G: entry offsets, points that cross each 128-byte block, keep and non-keep pieces
    for name in FORM:
        S = SCHEMAS[name]
        maxpt = min(S.max_regular, MAX_POINT)
        small = point_bytes(S, _ones(S))
        # pieces 1 and 2 are entered at offset e: a point of `size` bytes begins at 1024 + e - size, so the next begins at 1024 + e.
        # The smallest point for e = 0 and size - 1; the longest (every op's longest token) for e = 63, 64 and maxpt - 1 where the
        # form admits them (I64x6_2X8, 76 bytes: entries of 64 and more are the second candidate set's)
        longest = [S.max_len(o) for o in S.var_ops]
        entries = [(0, _ones(S)), (small - 1, _ones(S))] + ([(63, longest), (64, longest), (maxpt - 1, longest)] if maxpt > 64 else [])
        for e, pt in entries:
            def fn(a0, S=S, e=e, pt=pt):
                size = point_bytes(S, pt)
                return compose(a0, S, [("point", PIECE + e - size, pt), ("point", 2 * PIECE + e - size, pt)], more=100)
            # e >= 64 is read from the SECOND candidate set at lane e - 64. The first set's candidate in that lane, from offset
            # e - 64, must not arrive where the true one does, or the choice between the sets would not show: raw fields of 0xff
            # bytes end no varint, so a candidate that is not on a point's first byte dies in them
            def pred(M, a0, e=e):
                m = M[0]
                ok = m.entry[1] == e and m.entry[2] == e and m.candidate_exit(1, e) == e
                return ok and (e < 64 or m.candidate_exit(1, e - 64) != e)
            T.append(Row("entry_offset_%d_%s" % (e, name), "G", name, _one(fn), pred, a0s=(4, 15),
                         raw=(lambda i, b: 0xFF + 0 * i) if e >= 64 else bytes_any))

        def fn(a0, S=S):
            return compose(a0, S, [("point", PIECE + 128 * b - 3, [2] * len(S.var_ops)) for b in range(1, 8)], more=300)
        T.append(Row("points_cross_every_128_byte_block_" + name, "G", name, _one(fn),
                     all_of(*[point_at(PIECE + 128 * b - 3) for b in range(1, 8)])))
        assert maxpt <= MAX_POINT
    # keep: a form has more than 16 states, so a point has 17 bytes or more and a piece at most 60 points; only plans with 64 value
    # bytes per point and points of 18 bytes or less (I64_5B_R4_X8) have pieces that are not kept. One cloud: two pieces of the
    # smallest points, then long ones
    for name in FORM:
        S = SCHEMAS[name]

        def fn(a0, S=S):
            small = [_ones(S)] * (2 * PIECE // point_bytes(S, _ones(S)))
            big_pt = [S.max_len(o) for o in S.var_ops]
            if any(S.ops[o][0] == LF32 for o in S.var_ops):
                big_pt = [4 if S.ops[o][0] == LF32 else S.max_len(o) for o in S.var_ops]
            big = [big_pt] * (2 * PIECE // point_bytes(S, big_pt) + 2)
            return small + big + [_ones(S)] * 5
        T.append(Row("small_and_long_points_" + name, "G", name, _one(fn),
                     lambda M, a0, S=S: M[0].n_pieces >= 4 and bool(M[0].keep.any()) and (S.name != "I64_5B_R4_X8" or not M[0].keep[0])))


def _fixed_rows(T):
    # H: n around the tile of 1024 points, a full chunk; XOR values whose running value returns to 0 inside a tile
    for name in FIXED:
        S = SCHEMAS[name]
        for n in (1, 1023, 1024, 1025, 2047, 2048, 2049, CHUNK):
            T.append(Row("fixed_n_%d_%s" % (n, name), "H", name, _one(lambda a0, n=n: [[]] * n),
                         lambda M, a0, n=n, S=S: M[0].n == n and len(M[0].payload) == n * S.raw_bytes, a0s=(4, 9)))
        T.append(Row("fixed_xor_returns_to_0_" + name, "H", name, _one(lambda a0: [[]] * 3000),
                     lambda M, a0: M[0].n == 3000, raw=bytes_xor_returns))
        T.append(Row("fixed_runs_of_00_7f_80_ff_" + name, "H", name, _one(lambda a0: [[]] * 1500), lambda M, a0: M[0].n == 1500, raw=bytes_edges))


def _section_rows(T):
    # S: DeltaVarint sections (mode forced) of one and of two integer fields behind a bitmap-mode stream, through the side-by-side
    # route: the stream kernel in section mode, one integer op, MSB ends, the section's own a0. Predicates read every section's mode
    # byte and tokens (section_models). 64-bit fields cannot come here: narrow_fields (bpv <= 4) keeps them off this route.
    def walk16(k, i):
        return (np.cumsum(np.where(i % 5 == 0, 9000, np.where(i % 3 == 0, -70, 1))) % 60000)

    def walk32(k, i):
        step = np.array([1, -1, 100, -9000, 1 << 20, -(1 << 21), 1 << 27, 1 << 30], dtype=np.int64)[(i * 7 + i // 8) % 8]
        return np.cumsum(step) % (1 << 32)

    def all_dv(M, a0):
        return all(section_models(m) is not None for m in M)
    for name, ints, tops in (("XYZ_R4_U32", walk32, (5,)), ("XYZ_R4_U16_U32", lambda k, i: walk16(k, i) if k == 0 else walk32(k, i), (3, 5))):
        S = SCHEMAS[name]
        for n, span in ((300, lambda k: k == 1), (3000, lambda k: 2 <= k <= 32), (CHUNK + 500, lambda k: k > 32)):
            def pred(M, a0, n=n, span=span, tops=tops):
                secs = section_models(M[0])
                return sum(m.n for m in M) == n and all(set(sm.lens.tolist()) >= set(range(1, top + 1)) for sm, top in zip(secs, tops)) and \
                    span(secs[-1].n_pieces)
            T.append(Row("dv_sections_n_%d_%s" % (n, name), "S", name,
                         _one(lambda a0, S=S, n=n: [[1 + (q + o) % 2 for o in range(len(S.var_ops))] for q in range(n)]),
                         all_of(all_dv, pred), ints=ints, modes=[0] * len(S.adaptive)))

        # piece edges, as in family B: in the FIRST field's section a token of L bytes with s = 0..L of its bytes in front of a piece
        # edge (s = L: it ends at byte 1023; s = 0: it begins at 1024), edge after edge; the chunk at all 16 a0, so the section's own
        # a0 takes every value. The regular stream is 1-byte tokens (7 bytes a point), so the section begins at payload byte 7 n + 1:
        # 1-byte tokens are appended until that is the residue the tokens were laid out for.
        top = tops[0]
        for L in range(1, top + 1):
            def tokens(a0, L=L, top=top):
                want = 4
                pts = compose(want, SCHEMAS["I32"], [("point", (k + 1) * PIECE - sb, [L]) for k, sb in enumerate(range(L + 1))], more=40, long_ok=top)
                toks = [pt[0] for pt in pts]
                while (a0 + 7 * len(toks) + 1) % 16 != want:
                    toks.append(1)
                return toks

            def pred(M, a0, L=L):
                sm = section_models(M[0])[0]
                return sm.a0 == 4 and all(token_ends_at((k + 1) * PIECE - sb + L - 1, L)([sm], a0) for k, sb in enumerate(range(L + 1)))
            T.append(Row("dv_section_token_of_%d_bytes_at_piece_edges_%s" % (L, name), "S", name,
                         _one(lambda a0, S=S, tokens=tokens: [_ones(S)] * len(tokens(a0))), all_of(all_dv, pred), a0s=tuple(range(16)),
                         ints=ints, sect=lambda a0, n, tokens=tokens: {0: column(tokens(a0), INT, 4)}, modes=[0] * len(S.adaptive)))


def _table():
    T = []
    _length_rows(T)
    _edge_rows(T, ("F2", "XYZ_D"), "B", tuple(range(16)))
    _edge_rows(T, ("F1", "F8", "I64x8"), "B", (4,))
    _halo_rows(T)
    _piece_count_rows(T)
    _count_rows(T)
    _marker_rows(T)
    _regend_rows(T)
    _edge_rows(T, BITMAP, "F", tuple(range(16)))
    _edge_rows(T, FORM, "G", tuple(range(16)))
    _raw_rows(T)
    _form_rows(T)
    _fixed_rows(T)
    _section_rows(T)
    return T


ROWS = _table()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
HANDBACK = []      # (see the docstring: no well-formed chunk of these routes is handed back by design)
FAMILIES = ("A", "B", "C", "D", "E", "F", "G", "H", "S")


# ---------------------------------------------------------------------------------------------------------------------
# the route of a schema, through decode_route() itself (the shim of tests/test_decode_route.py)
# ---------------------------------------------------------------------------------------------------------------------
def selected_route(TR, lib, fields, step, version, enc, n_chunks=1):
    """(kernels, scalar fields) that decode_route() gives for the plan of these fields and a call of n_chunks chunks. The DecodeFacts
    are test_decode_route.abi_facts' restatement of what decode_framed fills in."""
    ops, adaptive, v5 = plan_of(fields, version, enc)
    r = TR.row("stream_grid", None, step, [(k, s, o) for k, s, o, _i in ops], [(b, o) for b, o, _i in adaptive], v5=1 if v5 else 0,
               n_chunks=n_chunks)
    return TR.route_of(lib, r)


def check_route(TR, lib, S, n_chunks=1):
    kernels, got = selected_route(TR, lib, S.fields, S.step, S.version, S.enc, n_chunks)
    assert (got["regular"], got["marker"], got["sections"]) == (S.route, S.marker, S.sections), (S.name, got)
    assert ("k_decode_fixed" if S.route == "fixed" else "k_decode_stream_w") in kernels
    if S.route in ("stream", "stream_cols"):
        assert got["redo"] == "any" and got["redo_only"] == 1
    else:
        assert got["redo"] == "none"
    return kernels, got
