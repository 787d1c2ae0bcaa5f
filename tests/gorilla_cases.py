"""The case table of tests/test_gorilla_model.py (CPU) and tests/test_gpu_gorilla.py: clouds whose Gorilla-coded doubles are built
from CHOSEN tokens (gorilla_model.values_for), and chunks written token by token for the forms only a decoder sees. Every row
carries a predicate on the model's token list / piece layout that proves the row is what its name says; the CPU test evaluates it.
DESIGN.md section 4 ("The Gorilla grid") has the table in words.

Padding is made of known lengths: a constant float lane is the 1-byte varint 0x01, a '0' token 1 byte, a '10' token under a window of
at most 6 bits 1 byte, a '11' token of at most 3 meaningful bits 2 bytes. With the stream at a 16-byte aligned device address the
payload of a cloud's first chunk lies at address 4 (mod 16): A0 below. The decoder's pieces are the addresses [1024 p, 1024 p + 1024).
"""
from __future__ import annotations

import numpy as np

import cases
import gorilla_model as GM

F = cases.F
RES = 0.001
A0 = 4
CHUNK = GM.CHUNK
LOSSY, LOSSLESS = cases.EncodingOptions.LOSSY, cases.EncodingOptions.LOSSLESS

_XYZ = [("x", 0, F.FLOAT32, RES), ("y", 4, F.FLOAT32, RES), ("z", 8, F.FLOAT32, RES)]
# name -> (fields, point step, encoding, ops of the regular stream, Gorilla fields, encoder pipelines, points of an encoder piece)
SCHEMAS = {
    "A": ([("x", 0, F.FLOAT32, RES), ("g", 4, F.FLOAT64, None)], 12, LOSSY, ["v", "g"], ["g"], (1,), 0),
    "B": (_XYZ + [("g", 12, F.FLOAT64, None)], 20, LOSSY, ["v", "v", "v", "g"], ["g"], (1, 2), 504),
    "B21": (_XYZ + [("g", 12, F.FLOAT64, None)], 21, LOSSY, ["v", "v", "v", "g"], ["g"], (1, 2), 504),   # every misalignment of the double
    "C": (_XYZ + [("intensity", 12, F.FLOAT32, RES), ("ring", 16, F.UINT16, None), ("g", 18, F.FLOAT64, None)], 26, LOSSY,
          ["v", "v", "v", "v", "g"], ["g"], (1, 2), 378),
    "D": ([("x", 0, F.FLOAT32, RES), ("a", 4, F.FLOAT64, None), ("b", 12, F.FLOAT64, None)], 20, LOSSY, ["v", "g", "g"], ["a", "b"], (1,), 0),
    "E": ([("a", 0, F.FLOAT64, None), ("f", 8, F.FLOAT32, None), ("b", 12, F.FLOAT64, None), ("k", 20, F.UINT8, None)], 21, LOSSLESS,
          ["g", ("r", 4), "g", ("r", 1)], ["a", "b"], (1,), 0),
    # 65 per-point tokens: the WIDE route (k_gorilla_tokens once per group of ops); the rows' values are in the 65th double
    "W": ([("g%d" % k, 8 * k, F.FLOAT64, None) for k in range(65)], 520, LOSSY, ["g"] * 65, ["g%d" % k for k in range(65)], (0,), 0),
}
_MAG = {1: 0, 2: 100, 3: 10_000, 4: 1 << 22, 5: 1 << 30}   # ticks of lane x that give a varint of that many bytes
FIRST = 0x3FF0000000000000


def ticks(values, scalar):
    """What the reference's float encoders quantise float32 values to at RES: value * (1 / RES) in float32, rounded (FloatN lanes:
    to nearest even, int32; a scalar FieldEncoderFloat_Lossy<float>: roundf, int64)."""
    v = np.asarray(values, dtype=np.float32)
    mult = np.float32(1.0 / float(np.float32(RES))) if scalar else np.float32(1.0) / np.float32(RES)
    t = (v * mult).astype(np.float32).astype(np.float64)
    return (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int64) if scalar else np.rint(t).astype(np.int64)


def x_lane(xlen, n):
    """Lane x of n points whose varints have the lengths xlen (default: 1 byte each): the value toggles between 0 and the magnitude
    of the length. -> float32[n]"""
    ln = np.ones(n, dtype=np.int64) if xlen is None else np.asarray(xlen, dtype=np.int64)
    assert len(ln) == n
    q = np.zeros(n, dtype=np.int64)
    for size, mag in _MAG.items():
        if size != 1:
            q += (np.cumsum(ln == size) % 2) * mag
    return (q.astype(np.float64) * RES).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# token specifications
# ---------------------------------------------------------------------------------------------------------------------
ZERO = ("0",)
REUSE = ("10", None)


def opener(clz, ctz, payload=None):
    return ("11", clz, ctz, payload)


def narrowing(k, skip=0):
    """k '11' specifications, each opening a window the one before does not hold: leading 31, 30, ... and three trailing counts per
    level (63 - l, 62 - l, 61 - l: 1, 2, 3 meaningful bits -- every token 2 bytes). 96 at most."""
    out = []
    for lead in range(31, -1, -1):
        for trail in (63 - lead, 62 - lead, 61 - lead):
            out.append(opener(lead, trail))
    assert skip + k <= len(out), "no more than 96 narrowing windows"
    return out[skip:skip + k]


def with_openers(n, positions, fill=REUSE, first_open=True):
    """Specifications of points 1 .. n - 1: `fill` everywhere, the next narrowing '11' at the points of `positions` (and at point 1,
    so that a window exists)."""
    pos = sorted(set(positions) | ({1} if first_open else set()))
    assert all(1 <= p < n for p in pos), (n, pos)
    ops = iter(narrowing(len(pos)))
    at = set(pos)
    return [next(ops) if i in at else fill for i in range(1, n)]


# ---------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, name, family, schema, chunks=None, xlen=None, hand=None, serial=0, pred=None, encode=True, error=None, note="",
                 decode=True):
        self.name, self.family, self.schema, self.xlen, self.serial, self.pred, self.note = name, family, schema, xlen, serial, pred, note
        self.chunks = chunks          # [chunk][Gorilla field] = (first value, specifications); None for hand-written rows
        self.hand = hand              # [(payload bytes, points)] per chunk, written token by token
        self.error = error            # malformed rows: 'corrupt' | 'truncated'
        self.encode = encode and hand is None
        self.decode = decode          # False: not a MODE 2 layout (WIDE): the hand-over model does not apply, encode only
        fields, self.step, self.enc, self.ops, self.gnames, self.pipelines, self.piece_pts = SCHEMAS[schema]
        self.fields = fields
        if hand is None:
            self.ns = [1 + len(c[0][1]) for c in chunks]
            assert all(1 + len(s) == n for c, n in zip(chunks, self.ns) for _f, s in c)
        else:
            self.ns = [n for _p, n in hand]
        assert all(n == CHUNK for n in self.ns[:-1]) and 1 <= self.ns[-1] <= CHUNK and len(self.ns) <= 3
        self.n = sum(self.ns)

    def info(self, n=None):
        return cases.make_info(self.fields, self.step, self.n if n is None else n, enc=self.enc)

    def bits(self):
        """Per Gorilla field the bit patterns of the whole cloud."""
        return [np.concatenate([GM.values_for(c[g][1], c[g][0]) for c in self.chunks]) for g in range(len(self.gnames))]

    def columns(self):
        n = self.n
        cols = {f[0]: np.zeros(n, dtype=cases._NP[f[2]]) for f in self.fields}
        if "x" in cols:
            cols["x"] = x_lane(self.xlen, n)
        if self.schema == "E":
            i = np.arange(n, dtype=np.uint64)
            cols["f"] = ((i * 0x01010101 + 0x80C0E0F0) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
            cols["k"] = ((i * 37 + 0x83) & 0xFF).astype(np.uint8)
        for name, b in zip(self.gnames, self.bits()):
            cols[name] = b.view(np.float64)
        return cols

    def cloud(self):
        return cases.pack(self.info(), self.columns(), self.n)

    def model_payloads(self):
        """The regular stream of every chunk as the model writes it (expressible rows)."""
        cols = self.columns()
        out, p0 = [], 0
        for n in self.ns:
            toks = []
            for o, (kind, f) in enumerate(zip(self.ops, [f for f in self.fields if f[0] != "ring"])):
                c = cols[f[0]][p0:p0 + n]
                if kind == "v":
                    q = ticks(c, scalar=self.schema in ("A", "D"))
                    d = np.diff(np.concatenate([[0], q]))
                    toks.append([GM.varint(int(x)) for x in d])
                elif kind == "g":
                    toks.append(GM.encode_tokens(c.view(np.uint64)))
                else:
                    u = c.view(np.uint32 if kind[1] == 4 else np.uint8).astype(np.uint64)
                    x = u ^ np.concatenate([[0], u[:-1]]).astype(np.uint64) if kind[1] == 4 else u
                    toks.append([int(v).to_bytes(kind[1], "little") for v in x])
            out.append(GM.regular_stream(self.ops, n, toks))
            p0 += n
        return out

    def stream(self, oracle):
        if self.hand is None:
            return oracle.encode_stage1(self.info(), self.cloud())
        return frame([p for p, _n in self.hand])


def frame(payloads):
    return np.concatenate([np.concatenate([np.frombuffer(np.uint32(len(p)).tobytes(), np.uint8), np.frombuffer(bytes(p), np.uint8)])
                           for p in payloads])


def split_chunks(stream):
    """[(payload offset in the stream, payload)]"""
    s, pos, out = np.asarray(stream, dtype=np.uint8), 0, []
    while pos < len(s):
        size = int(np.frombuffer(s[pos:pos + 4].tobytes(), "<u4")[0])
        out.append((pos + 4, s[pos + 4:pos + 4 + size]))
        pos += 4 + size
    return out


def layout(row, stream, residue=0):
    """Per chunk (parsed regular stream, serial, reason, pieces) with the stream at device address `residue` (mod 16)."""
    out = []
    for (off, payload), n in zip(split_chunks(stream), row.ns):
        P = GM.parse_regular(payload, row.ops, n)
        out.append((P,) + GM.serial_expected(payload, (residue + off) % 16, row.ops, n, parsed=P))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# predicates: pred(L) with L = layout(row, stream): the list of (P, serial, reason, pieces) per chunk
# ---------------------------------------------------------------------------------------------------------------------
def kinds_are(expected, chunk=0, g=0, at=1):
    return lambda L: L[chunk][0].kinds[g][at:at + len(expected)] == list(expected)


def opens_at(positions, chunk=0, g=0):
    """'11' tokens exactly at `positions` (every one a different window), nowhere else."""
    def pred(L):
        P = L[chunk][0]
        return [i for i, k in enumerate(P.kinds[g]) if k == "11"] == sorted(positions) and all(P.changed[i] for i in positions)
    return pred


def address_of(point, address, chunk=0):
    return lambda L: A0 + L[chunk][0].start[point] == address


def piece_changes(expected, chunk=0):
    """{piece: changing points it owns} for the named pieces"""
    return lambda L: all(next(p for p in L[chunk][3] if p.index == k).changes == v for k, v in expected.items())


def _second_value_fits_the_window_before(L):
    """Every chunk's second token is a '11'; from the second chunk on its difference has at least the leading and trailing zeros
    of the window the chunk before ended under, (12, 12) -- with the state carried over it would have been a '10'."""
    for k, c in enumerate(L):
        P = c[0]
        if len(P.start) < 2:
            continue
        if P.kinds[0][1] != "11":
            return False
        if k:
            x = int(P.values[0][0]) ^ int(P.values[0][1])
            w = L[k - 1][0].wins[-1][0]
            if w != (12, 12) or GM.clz64(x) < w[0] or GM.ctz64(x) < w[1]:
                return False
    return True


def both(*preds):
    return lambda L: all(p(L) for p in preds)


# ---------------------------------------------------------------------------------------------------------------------
def one(first, specs, fields=1):
    return [[(first ^ (0x1111 * g), specs) for g in range(fields)]]


def _every_length():
    """Family a: '11' tokens of every m at stored leading 31, at the largest leading m allows and at leading 0 (in this order every
    one opens: trailing falls under leading 31, then leading falls, then (0, 63) is below leading 1 and trailing falls again), each
    followed by a '10' under the window it opened and a repeat."""
    seq = [(31, 33 - m) for m in range(1, 34)] + [(64 - m, 0) for m in range(34, 64)] + [(0, 64 - m) for m in range(1, 65)]
    specs = []
    for lead, trail in seq:
        specs += [opener(lead, trail), REUSE, ZERO] + [ZERO] * 15     # (16 repeats: fewer than 40 changing points in any KiB)
    return specs, seq


def _pad_a(address, xlen, cur=A0 + 9):
    """Schema A: repeats (2-byte points; one 3-byte point, its varint 2 bytes, for the parity) from address `cur` (behind the 9-byte
    first point unless given) so that the next point begins at `address`. Appends the varint lengths to xlen, returns the specifications."""
    gap = address - cur
    assert gap >= 0 and gap != 1, gap
    odd = gap % 2
    count = (gap - 3 * odd) // 2 + odd
    xlen += [2] * odd + [1] * (count - odd)
    return [ZERO] * count


def _xl(xl, specs):
    """varint lengths of all points: those chosen so far, 1 byte for the rest"""
    return (xl + [1] * (len(specs) + 1))[:len(specs) + 1]


def _table():
    T = []
    fams = {"A": 1, "B": 1, "B21": 1, "C": 1, "D": 2, "E": 2}
    # ---- a: every token length, in one cloud per schema
    specs, seq = _every_length()
    for s, nf in fams.items():
        T.append(Row("a_every_length_" + s, "a", s, one(FIRST, specs, nf),
                     pred=lambda L, seq=seq: L[0][0].kinds[0][1:] == (["11", "10"] + ["0"] * 16) * len(seq)
                     and [w[0] for w in L[0][0].wins[1::18]] == [(min(a, 31), b) for a, b in seq]))
    # ---- b: the clamp of the stored leading count: clz 30, 31, 32, 63 open, a value with clz 40 and the same ctz reuses (31, T)
    for s in ("A", "B", "C"):
        for lead in (30, 31, 32, 63):
            trail = 0 if lead == 63 else 3
            sp = [opener(lead, trail), ("10", GM.default_payload(24 - trail)), ZERO, ("10", GM.default_payload(24 - trail) ^ 2 ^ (1 << 5))]
            T.append(Row("b_clamp_clz%d_%s" % (lead, s), "b", s, one(FIRST, sp),
                         pred=both(kinds_are(["11", "10", "0", "10"]), lambda L, w=(min(lead, 31), trail): L[0][0].wins[4][0] == w)))
    # ---- c: reuse edges under the window (12, 12): exact on both sides; clz = L - 1; ctz = T - 1; a repeat behind an opener
    for s in ("A", "B", "C", "D", "E"):
        sp = [opener(12, 12), REUSE, ("10", GM.default_payload(40) | 0xF0), opener(11, 20), ZERO, REUSE, opener(15, 19), ZERO, ZERO, REUSE,
              ("10", 1), ("10", 1 << 29)]
        T.append(Row("c_reuse_edges_" + s, "c", s, one(FIRST, sp, fams[s]),
                     pred=kinds_are(["11", "10", "10", "11", "0", "10", "11", "0", "0", "10", "10", "10"])))
    # ---- d: forms only a decoder sees, written by hand into schema A (x constant: the byte 0x01 in front of every token)
    w = (10, 20)

    def hand_a(tokens):
        return [(b"".join(b"\x01" + t for t in tokens), len(tokens))]
    pay = GM.default_payload(34)
    T.append(Row("d_reopen_same_window", "d", "A", hand=hand_a([GM.tok_first(FIRST), GM.tok_open(10, 34, pay), GM.tok_reuse(w, pay ^ 6), GM.tok_open(10, 34, pay ^ 0x30),
                                                               GM.tok_reuse(w, 5), GM.tok_repeat(), GM.tok_open(10, 34, 1 << 20), GM.tok_reuse(w, 7)]),
                 pred=lambda L: L[0][0].kinds[0][1:] == ["11", "10", "11", "10", "0", "11", "10"] and L[0][0].changed == [False, True] + [False] * 6))
    T.append(Row("d_leading_understated", "d", "A", hand=hand_a([GM.tok_first(FIRST), GM.tok_open(5, 20, 0x00123), GM.tok_reuse((5, 39), 0x7FFFF), GM.tok_repeat()]),
                 pred=kinds_are(["11", "10", "0"])))
    T.append(Row("d_payload_lowest_bit_zero", "d", "A", hand=hand_a([GM.tok_first(0), GM.tok_open(5, 20, 0x80000), GM.tok_open(31, 1, 0), GM.tok_reuse((31, 32), 0), GM.tok_reuse((31, 32), 1)]),
                 pred=kinds_are(["11", "11", "10", "10"])))
    T.append(Row("d_77_bits", "d", "A", hand=hand_a([GM.tok_first(GM.M64), GM.tok_open(0, 64, GM.M64), GM.tok_open(0, 64, 0x8000000000000001), GM.tok_reuse((0, 0), 0x1234567890ABCDEF),
                                                    GM.tok_repeat(), GM.tok_open(0, 64, 1)]),
                 pred=lambda L: L[0][0].size[1:] == [11, 11, 10, 2, 11] and L[0][0].changed[1:] == [True, False, False, False, False]))
    T.append(Row("d_padding_bits_set", "d", "A", hand=hand_a([GM.tok_first(FIRST), GM.tok_open(10, 34, pay, pad=0xFF), GM.tok_reuse(w, pay ^ 6, pad=0xFF), GM.tok_repeat(pad=0x7F),
                                                             GM.tok_repeat(pad=0x55), GM.tok_open(31, 2, 3, pad=0xFF), GM.tok_reuse((31, 31), 2, pad=0xFF), GM.tok_repeat(pad=1)]),
                 pred=kinds_are(["11", "10", "0", "0", "11", "10", "0"])))
    # ---- e: the raw first value (bytes that read as tokens), the smallest clouds; the GPU test places them at all 16 residues
    for name, first in (("00", 0), ("ff", GM.M64), ("03", 0x0300000000000003), ("01", 0x0101010101010101)):
        T.append(Row("e_first_" + name, "e", "A", one(first, [opener(0, 0), REUSE]), pred=kinds_are(["11", "10"])))
        T.append(Row("e_first_%s_C" % name, "e", "C", one(first, [opener(20, 20), ZERO]), pred=kinds_are(["11", "0"])))
    for n in (1, 2, 3):
        T.append(Row("e_n%d" % n, "e", "A", one(GM.M64 ^ 1, [opener(1, 0), ZERO][:n - 1]), pred=lambda L, n=n: len(L[0][0].start) == n))
        T.append(Row("e_n%d_D" % n, "e", "D", one(3, [opener(1, 0), REUSE][:n - 1], 2), pred=lambda L, n=n: len(L[0][0].start) == n))
    # ---- f: piece boundaries of the decoder (schema A; addresses are counted from the payload's address - A0)
    for d in range(1, 11):   # the 10-byte '11' token (m = 64) begins d bytes in front of address 1024: its point one byte earlier
        xl = [1]
        sp = _pad_a(1024 - d - 1, xl)
        k = len(sp) + 1
        sp += [opener(0, 0), REUSE, ZERO, REUSE] + [ZERO] * 40
        T.append(Row("f_ten_bytes_%d_in_front" % d, "f", "A", one(FIRST, sp), xlen=_xl(xl, sp),
                     pred=both(address_of(k, 1023 - d), lambda L, k=k: L[0][0].size[k] == 11 and L[0][0].changed[k])))
    for what, addr in (("last_byte", 1023), ("first_byte", 1024), ("second_byte", 1025)):
        # a window exists; the point at `addr` changes it: the last point piece 0 owns / the first of piece 1 / one byte behind a
        # fourth point that ended one byte past the boundary
        xl = [1, 1]
        sp = [opener(31, 32)]
        sp += _pad_a(addr, xl, cur=A0 + 9 + 3)
        k = len(sp) + 1
        sp += [opener(20, 20), REUSE, ZERO, REUSE] + [ZERO] * 40
        T.append(Row("f_changing_point_on_" + what, "f", "A", one(FIRST, sp), xlen=_xl(xl, sp),
                     pred=both(address_of(k, addr), lambda L, k=k: L[0][0].changed[k])))
    # changes in pieces 15, 16, 17 (the ring of 16 chain records wraps), and one in every piece of 32 (every guess is stale):
    # 2-byte points, 512 to a piece
    n = 18 * 512 + 100
    T.append(Row("f_changes_in_pieces_15_16_17", "f", "A", one(FIRST, with_openers(n, [15 * 512 + 7, 16 * 512 + 300, 17 * 512 + 500], fill=ZERO)),
                 pred=piece_changes({0: 1, 14: 0, 15: 1, 16: 1, 17: 1})))
    n = 32 * 512 + 9
    T.append(Row("f_change_in_every_piece", "f", "A", one(FIRST, with_openers(n, [p * 512 + 37 * p % 400 + 3 for p in range(32)], fill=ZERO)),
                 pred=lambda L: [p.changes for p in L[0][3][:32]] == [2] + [1] * 31))
    # ---- g: hop4 -- the changing point k points behind the first point piece 1 owns
    for k in range(1, 6):
        xl = [1, 1]
        sp = [opener(31, 32)]
        sp += _pad_a(1024, xl, cur=A0 + 9 + 3)
        e = len(sp) + 1                      # the point at address 1024
        sp += [REUSE] * (k + 1)
        sp[e - 1 + k] = opener(20, 20)
        sp += [REUSE, ZERO] * 30
        T.append(Row("g_change_%d_behind_the_entry" % k, "g", "A", one(FIRST, sp), xlen=_xl(xl, sp),
                     pred=both(address_of(e, 1024), lambda L, e=e, k=k: L[0][0].changed[e + k] and not any(L[0][0].changed[e:e + k]))))
    # the fourth point from a piece's entry -- and so every fourth point behind it, 128 hops -- ends exactly on the piece's end / one byte
    # past it: pieces 1..14 own 512 two-byte points each, none changes the window (settled at point 1, so from piece 12 on -- a
    # wave's second piece -- the guess is right whatever the timing: no rounds), the candidate walk leaves through hop4 = kSwPiece
    # / kSwPiece + 1 (step 3 of make_jt_gor: `e < 0x8000u`), the record's entry is 0 / 1
    for what, first in (("on_the_boundary", 1024), ("one_byte_past_the_boundary", 1025)):
        xl = [1, 1]
        sp = [opener(31, 32)]
        sp += _pad_a(first, xl, cur=A0 + 9 + 3)
        sp += [REUSE, ZERO, ZERO, REUSE, REUSE, ZERO, REUSE] * (15 * 512 // 7)
        T.append(Row("g_every_fourth_point_ends_" + what, "g", "A", one(FIRST, sp), xlen=_xl(xl, sp),
                     pred=lambda L, first=first: all(q.index == k and q.npts == 512 and q.changes == 0 and A0 + L[0][0].start[q.first_point] == 1024 * k + first - 1024
                                                     and L[0][0].size[q.first_point + q.npts - 1] == 2 for k, q in enumerate(L[0][3]) if 1 <= k <= 14)
                     and len(L[0][3]) >= 16 and L[0][3][0].changes == 1))
    # the fewest points a piece can own: schema D by hand, a 5-byte varint and two 10-byte '11' tokens (the same window (0, 0) again
    # and again: no encoder writes that) -- 25 bytes per point, 40 or 41 points per piece
    rs = np.random.RandomState(3)
    toks = [GM.varint(0) + GM.tok_first(1) + GM.tok_first(2)]
    for i in range(1, 260):
        a, b = (int(rs.randint(0, 1 << 62)) << 2 | 1, int(rs.randint(0, 1 << 62)) << 1 | (1 << 63))
        toks.append(GM.varint((1 << 30) * (1 if i % 2 else -1)) + GM.tok_open(0, 64, a) + GM.tok_open(0, 64, b))
    T.append(Row("g_fewest_points_per_piece_D", "g", "D", hand=[(b"".join(toks), len(toks))],
                 pred=lambda L: all(s == 25 for s in L[0][0].size[1:]) and L[0][0].changed[1] and not any(L[0][0].changed[2:])
                 and {p.npts for p in L[0][3][1:-1]} <= {40, 41}))
    # ---- h: the rounds cap. k changing points (3 bytes each) in piece 0 (directly behind the first value) / in piece 1
    for where, piece in (("first_piece", 0), ("second_piece", 1)):
        for k, last, serial in ((38, False, 0), (39, False, 0), (40, False, 1), (41, False, 1), (40, True, 0)):
            # last: the 40th changing point begins two bytes in front of the piece's end -- it is the last point the piece owns and
            # the loop leaves before the cap is looked at
            at = 1024 * (piece + 1) - 3 * k + 1 if last else (A0 + 9 if piece == 0 else 1024)
            xl = [1]
            sp = _pad_a(at, xl)
            sp += narrowing(k) + [ZERO] * 6 + [REUSE] * 3 + [ZERO] * 20
            name = "h_%d_changes_in_the_%s%s" % (k, where, "_the_last_its_last_point" if last else "")
            T.append(Row(name, "h", "A", one(FIRST, sp), xlen=_xl(xl, sp), serial=serial,
                         pred=lambda L, k=k, p=piece: next(q for q in L[0][3] if q.index == p).changes == k))
    # 39 + 39 in two neighbouring pieces
    xl = [1]
    sp = _pad_a(1024 - 3 * 39, xl)
    sp += narrowing(78) + [ZERO] * 10
    T.append(Row("h_39_and_39_in_neighbouring_pieces", "h", "A", one(FIRST, sp), xlen=_xl(xl, sp),
                 pred=piece_changes({0: 39, 1: 39})))
    # ---- i: chunk boundaries: the second value of chunk k + 1 would fit chunk k's last window (12, 12): a new chunk has none
    for s in ("A", "C"):
        for n_chunks, last in ((2, 40), (3, 40), (1, CHUNK), (2, 1)):
            ch = []
            for c in range(n_chunks):
                n = last if c == n_chunks - 1 else CHUNK
                sp = ([opener(12, 12)] + [REUSE, ZERO, REUSE, REUSE] * ((n - 2) // 4 + 1))[:n - 1]
                ch.append([(FIRST + 0x1000 * c, sp)])
            name = "i_%d_chunks_%s" % (n_chunks, s) if last == 40 else "i_n%d_%s" % ((n_chunks - 1) * CHUNK + last, s)
            T.append(Row(name, "i", s, ch, pred=_second_value_fits_the_window_before))
    # ---- j: encoder geometry (batches of 64 points, the load layout k * 512 + tid, passes of 8192, pieces of 504 / 378, rows of 63)
    geo = [("openers_62_65", 200, [62, 63, 64, 65]), ("openers_511_513", 700, [511, 512, 513]),
           ("openers_8190_8193", 8300, [8190, 8191, 8192, 8193]),
           ("piece_edges", 2100, sorted({q + d for q in (378, 756, 1890, 504, 1008, 1512, 2016) for d in (-2, -1, 0, 1, 2)})),
           ("piece_rows_lane_1_and_63", 1100, [378, 378 + 62, 378 + 63, 378 + 125, 504, 504 + 62, 504 + 63, 504 + 125]),
           ("2_in_a_batch", 300, [130, 190]), ("3_in_a_batch", 300, [128, 160, 191]), ("63_in_a_batch", 300, list(range(129, 192)))]
    for s in ("A", "B", "B21", "C"):
        for what, n, pos in geo:
            # (63 changing points in a row lie within 400 bytes of stream: on the way back the decoder's rounds cap sends that chunk
            # to the serial decoder -- the only rows outside family h that do)
            T.append(Row("j_%s_%s" % (what, s), "j", s, one(FIRST, with_openers(n, pos)), serial=int(len(pos) == 63),
                         pred=opens_at(sorted(set(pos) | {1}))))
        # (the rows go on beyond the first boundary of both piece sizes: what the pre-pass made of the batch is published there)
        # a batch [128, 192) whose every difference has exactly the window's (12, 12) counts: quiet; one point with clz 11 / ctz 11: not
        base = [opener(12, 12)] + [ZERO] * 126
        T.append(Row("j_batch_equals_window_" + s, "j", s, one(FIRST, base + [REUSE] * 64 + [REUSE, ZERO] * 200), pred=opens_at([1])))
        T.append(Row("j_batch_one_less_leading_" + s, "j", s, one(FIRST, base + [REUSE] * 40 + [opener(11, 12)] + [REUSE] * 23 + [REUSE, ZERO] * 200),
                     pred=opens_at([1, 168])))
        T.append(Row("j_batch_one_less_trailing_" + s, "j", s, one(FIRST, base + [REUSE] * 63 + [opener(12, 11)] + [REUSE, ZERO] * 200),
                     pred=opens_at([1, 191])))
        T.append(Row("j_batch_of_repeats_" + s, "j", s, one(FIRST, [opener(12, 12)] + [REUSE] * 62 + [ZERO] * 64 + [REUSE] * 400),
                     pred=lambda L: L[0][0].kinds[0][64:128] == ["0"] * 64))
    # the clamp where the piece kernel takes its window from the pre-pass: clz 40 opens (31, 2), nothing but reuses with clz 42 across
    # the boundaries of both piece sizes -- 2 + 31 bits are 5 bytes, under a window (32, 2) they would be 4 -- and reuses with clz 31
    # exactly behind the last boundary (in front of it they would mend a wrong window: under (32, 2) they open (31, 2))
    for s in ("A", "B", "B21", "C"):
        sp = [opener(40, 2)] + [("10", GM.default_payload(20) ^ (i << 1)) if i < 1050 else REUSE for i in range(2, 1100)]
        T.append(Row("j_clamped_window_across_pieces_" + s, "j", s, one(FIRST, sp),
                     pred=both(opens_at([1]), lambda L: L[0][0].wins[-1][0] == (31, 2) and L[0][0].kinds[0][378] == L[0][0].kinds[0][504] == "10"
                               and all(GM.clz64(int(a) ^ int(b)) == 42 for a, b in zip(L[0][0].values[0][1:1049], L[0][0].values[0][2:1050])))))
    for what, n, pos in geo[:3] + geo[-1:]:      # the WIDE route: the same values in the 65th of 65 doubles, the others stand still
        ch = [[(FIRST + g, [ZERO] * (n - 1)) for g in range(64)] + [(FIRST, with_openers(n, pos))]]
        T.append(Row("j_%s_W" % what, "j", "W", ch, decode=False, pred=opens_at(sorted(set(pos) | {1}), g=64)))
    # ---- k: malformed chunks (decoder only, by hand, schema A)
    T.append(Row("k_reuse_without_a_window", "k", "A", hand=hand_a([GM.tok_first(FIRST), GM.tok_reuse((10, 20), 5), GM.tok_repeat()]), error="corrupt"))
    T.append(Row("k_window_of_more_than_64_bits", "k", "A", hand=hand_a([GM.tok_first(FIRST), GM.tok_open(10, 34, pay), GM.tok_open(20, 50, 1), GM.tok_repeat()]),
                 error="corrupt"))
    cut = hand_a([GM.tok_first(FIRST), GM.tok_open(10, 34, pay), GM.tok_reuse(w, 9), GM.tok_open(0, 64, 77)])
    T.append(Row("k_token_cut_off_by_the_end", "k", "A", hand=[(cut[0][0][:-4], 4)], error="truncated"))
    return T


ROWS = _table()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
EXPRESSIBLE = [r for r in ROWS if r.hand is None]
WELL_FORMED = [r for r in ROWS if r.error is None]
DECODE = [r for r in WELL_FORMED if r.decode]
MALFORMED = [r for r in ROWS if r.error is not None]
