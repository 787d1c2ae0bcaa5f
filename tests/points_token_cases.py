"""The case table of tests/test_points_token_cases.py (CPU) and tests/test_gpu_points_tokens.py: chunks whose FloatN token stream is
built from CHOSEN token lengths at CHOSEN positions, for k_decode_points_w (cloudini_amd/csrc/stage1_decode_wave.h). The oracle's
encoder writes every stream; every row carries a predicate on the bytes it wrote that proves the row is what its name says, and the
CPU test evaluates it at every address residue the GPU test uses the row at. DESIGN.md section 4 ("The point-decoder token grid")
has the table in words.

Token lengths are chosen through the deltas: a float lane at resolution 0.5 holds x = q * 0.5 with q a running sum of deltas
+-2^(7(L-1)-1) (0 for L = 1), whose token -- the varint of zigzag(delta) + 1 -- has exactly L bytes, L = 1..5. A NaN is the single
byte 0x00 and resets its lane's running value. Token codes in this file: 0 = the NaN marker, 1..5 = a token of that many bytes.

Positions are counted as the kernel's header comment counts them: v = payload offset + a0, a0 = the payload's address mod 16; piece p
is v in [992 p, 992 (p + 1)), cut into 62 units of 16 bytes (lanes 1..62), lane 0 the unit in front, lane 63 the halo. The piece model
below (`Model`) restates that comment in numpy; it is checked against a byte-by-byte walk by the CPU test and shares nothing with the
kernel's code path.
"""
from __future__ import annotations

import numpy as np

import cases

F = cases.F
PIECE = 992          # kWpPiece
UNIT = 16
UNITS = 62           # kWpUnits
RING = 64            # kWpRing
SLOTS = 1024         # kWpSlots
CHUNK = 32768
RES = 0.5


def _floats(names, first=0):
    return [(c, first + 4 * k, F.FLOAT32, RES) for k, c in enumerate(names)]


def _u16s(k, first):
    return [("i%d" % a, first + 2 * a, F.UINT16, None) for a in range(k)]


def _five_ints(first):
    return [("i0", first, F.UINT16, None), ("i1", first + 2, F.UINT16, None), ("i2", first + 4, F.UINT32, None),
            ("i3", first + 8, F.UINT32, None), ("i4", first + 12, F.UINT32, None)]


# name -> (fields, point step). The float lanes come first; NOPS = their number.
SCHEMAS = {
    "XYZ": (_floats("xyz"), 12),
    "XYZW": (_floats("xyzw"), 16),
    "XYZ_U16": (_floats("xyz") + _u16s(1, 12), 16),
    "XYZ_U32": (_floats("xyz") + [("i0", 12, F.UINT32, None)], 16),
    # the other variants of kPointsVariants (tests/test_gpu_points_tokens.py::test_every_points_variant)
    "XYZ_ODD": (_floats("xyz", 1), 13),
    "XYZ_U16_ODD": (_floats("xyz") + [("i0", 13, F.UINT16, None)], 16),
    "XYZ_2U16": (_floats("xyz") + _u16s(2, 12), 16),
    "XYZ_5INTS": (_floats("xyz") + _five_ints(12), 28),
    "XYZW_U16": (_floats("xyzw") + _u16s(1, 16), 20),
    "XYZW_2U16": (_floats("xyzw") + _u16s(2, 16), 20),
    "XYZW_5INTS": (_floats("xyzw") + _five_ints(16), 32),
}


def nops_of(schema):
    return sum(1 for f in SCHEMAS[schema][0] if f[3] is not None)


def int_fields(schema):
    return [f for f in SCHEMAS[schema][0] if f[3] is None]


# ---------------------------------------------------------------------------------------------------------------------
# token codes -> float lanes
# ---------------------------------------------------------------------------------------------------------------------
def lanes_for(codes, nops, signs=None):
    """float32 [n, nops] whose tokens have the codes `codes` (stream order: point-major). The k-th token of a length class in a lane
    goes up for even k and down for odd k, so every running value stays within a few powers of two; `signs` (same shape, +-1, 0 = the
    rule) overrides that."""
    c = np.asarray(codes, dtype=np.int64).reshape(-1, nops)
    n = len(c)
    out = np.empty((n, nops), dtype=np.float32)
    sg = None if signs is None else np.asarray(signs, dtype=np.int64).reshape(-1, nops)
    assert c.min(initial=1) >= 0 and c.max(initial=1) <= 5
    for o in range(nops):
        ln = c[:, o]
        mag = np.where(ln <= 1, 0, np.int64(1) << (7 * (ln - 1) - 1).clip(0))
        sgn = np.ones(n, dtype=np.int64)
        for k in range(2, 6):
            idx = np.nonzero(ln == k)[0]
            sgn[idx] = np.where(np.arange(len(idx)) & 1, -1, 1)
        if sg is not None:
            sgn = np.where(sg[:, o] != 0, sg[:, o], sgn)
        cs = np.cumsum(mag * sgn)
        nan = ln == 0
        last = np.maximum.accumulate(np.where(nan, np.arange(n), -1))
        q = cs - np.where(last >= 0, cs[last.clip(0)], 0)
        assert np.abs(q).max(initial=0) < (1 << 30)
        x = (q * RES).astype(np.float32)
        assert np.array_equal(x.astype(np.int64) * 2, q)       # exactly representable: the round trip is exact
        x[nan] = np.nan
        out[:, o] = x
    return out


def varint_len(x):
    n = 1
    while x >> (7 * n):
        n += 1
    return n


def fill(nbytes, r, nops):
    """token lengths (1..4, mixed) that sum to `nbytes`, their number congruent to r modulo nops"""
    if nbytes == 0:
        assert r % nops == 0, "no room for %d tokens" % r
        return []
    t = nbytes * 5 // 8
    t -= (t - r) % nops
    while 4 * t < nbytes:
        t += nops
    while t > nbytes:
        t -= nops
    assert t > 0 and t <= nbytes <= 4 * t, (nbytes, r, nops)
    e = nbytes - t
    ln = [1 + e // t + (1 if i < e % t else 0) for i in range(t)]
    ln = [ln[(i * 7) % t] for i in range(t)] if t % 7 else ln     # (a permutation: the longer tokens spread out)
    for i in range(0, t - 2, 5):                                   # some tokens of 3 and 4 bytes, sum and number kept
        if ln[i] == 2 and ln[i + 1] == 2 and ln[i + 2] == 2 and i % 2:
            ln[i:i + 3] = [4, 1, 1]
        elif ln[i] == 2 and ln[i + 1] == 2:
            ln[i:i + 2] = [3, 1]
    assert sum(ln) == nbytes and len(ln) % nops == r % nops and min(ln) >= 1 and max(ln) <= 4
    return ln


def _blen(code):
    return 1 if code == 0 else code


def compose(a0, nops, items, total=None, more=0):
    """Token codes of a chunk. items, in stream order: ("pin", V, code, o) = a token of that code, the o-th of its point (None: any),
    whose LAST byte lies at v = V; ("run", codes) = these tokens next. Mixed filler goes in between. Behind the last item the open
    point is completed; then `more` bytes of whole points follow, or filler up to a payload of exactly `total` bytes."""
    codes, off = [], 0
    for it in items:
        if it[0] == "run":
            codes += list(it[1])
            off += sum(_blen(c) for c in it[1])
            continue
        _pin, V, code, o = it
        start = V - a0 - (_blen(code) - 1)
        gap = start - off
        assert gap >= 0, (it, off)
        if o is None:
            for r in range(nops):
                try:
                    f = fill(gap, r, nops)
                    break
                except AssertionError:
                    f = None
            assert f is not None, (it, gap)
        else:
            f = fill(gap, o - len(codes), nops)
        codes += f + [code]
        off = start + _blen(code)
        assert o is None or (len(codes) - 1) % nops == o
    if total is not None:
        codes += fill(total - off, -len(codes), nops)
    else:
        while len(codes) % nops:
            codes.append(1)
        if more:
            codes += fill(more, 0, nops)
    assert len(codes) % nops == 0
    return codes


# ---------------------------------------------------------------------------------------------------------------------
# the piece model: the header comment of stage1_decode_wave.h in numpy
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    """Of one chunk. ends / lens / values: the regular stream's tokens (payload offset of the last byte, bytes, the varint's value
    u = zigzag + 1, 0 = NaN marker). reg_end: the payload offset behind them. Per piece p: T0[p] token ends in front of it and
    cnt[p] in it (as the kernel counts them: every payload byte with a clear MSB, section bytes included), owned[p] = (first, number)
    of the points whose FIRST token ends in it, halo_tokens[p] / halo_bytes[p] = how much of the last owned point lies behind the
    piece. Per point: owner piece and row (index among the piece's points // 64)."""

    def __init__(self, payload, a0, nops, n):
        p = np.asarray(payload, dtype=np.uint8)
        self.payload, self.a0, self.nops, self.n = p, a0, nops, n
        all_ends = np.nonzero(p < 0x80)[0]
        target = n * nops
        assert len(all_ends) >= target
        self.ends = all_ends[:target]
        self.lens = np.diff(self.ends, prepend=-1)
        self.reg_end = int(self.ends[-1]) + 1 if target else 0
        self.vend = a0 + len(p)
        self.n_pieces = (self.vend + PIECE - 1) // PIECE if len(p) else 0
        edges = np.arange(self.n_pieces + 1) * PIECE
        self.T0 = np.searchsorted(all_ends + a0, edges[:-1])
        self.cnt = np.searchsorted(all_ends + a0, edges[1:]) - self.T0
        v = self.ends + a0
        self.owner = v[0::nops] // PIECE if target else np.zeros(0, np.int64)
        first = np.searchsorted(self.owner, np.arange(self.n_pieces))
        number = np.searchsorted(self.owner, np.arange(self.n_pieces), side="right") - first
        self.owned = list(zip(first.tolist(), number.tolist()))
        self.row = (np.arange(n) - first[self.owner]) // 64 if n else np.zeros(0, np.int64)
        self.halo_tokens, self.halo_bytes = [], []
        for pc, (f, k) in enumerate(self.owned):
            if k == 0:
                self.halo_tokens.append(0)
                self.halo_bytes.append(0)
                continue
            tv = v[(f + k - 1) * nops:(f + k) * nops]
            self.halo_tokens.append(int(np.sum(tv >= (pc + 1) * PIECE)))
            self.halo_bytes.append(max(0, int(tv[-1]) - (pc + 1) * PIECE + 1))
        # values
        u = np.zeros(target, dtype=np.int64)
        for k in range(5):
            idx = self.ends - (self.lens - 1) + k
            take = k < self.lens
            u += np.where(take, (p[np.where(take, idx, 0)].astype(np.int64) & 0x7F) << (7 * k), 0)
        self.values = u
        self.markers = (u == 0)

    def token_v(self):
        return self.ends + self.a0

    def running(self):
        """int64 [n, nops]: every lane's running value behind each point (a marker resets its lane to 0)"""
        u1 = self.values - 1
        d = np.where(self.markers, 0, (u1 >> 1) ^ -(u1 & 1)).reshape(self.n, self.nops)
        mk = self.markers.reshape(self.n, self.nops)
        out = np.empty_like(d)
        for o in range(self.nops):
            cs = np.cumsum(d[:, o])
            last = np.maximum.accumulate(np.where(mk[:, o], np.arange(self.n), -1))
            out[:, o] = cs - np.where(last >= 0, cs[last.clip(0)], 0)
        return out

    def unit_positions(self):
        """{(place, position in the unit, length)} of the tokens of at most 4 bytes, pieces 1.. only; place = 1, 62 or 0 (a lane
        between)"""
        v = self.token_v()
        lane = (v % PIECE) // UNIT + 1
        place = np.where(lane == 1, 1, np.where(lane == UNITS, UNITS, 0))
        ok = (self.lens <= 4) & (v >= PIECE)
        return set(zip(place[ok].tolist(), (v[ok] % UNIT).tolist(), self.lens[ok].tolist()))

    def boundary_splits(self):
        """{(length, s, o)}: a token, the o-th of its point, with s of its bytes in front of a piece boundary (s = 0: it begins on the
        boundary, s = length: it ends on the piece's last byte)"""
        v = self.token_v()
        start = v - self.lens + 1
        b = (v + 1) // PIECE * PIECE                       # the boundary at or below the byte behind the token
        ok = (b >= start) & (b > 0) & (self.lens <= 5)
        o = np.arange(len(v)) % self.nops
        return set(zip(self.lens[ok].tolist(), (b - start)[ok].tolist(), o[ok].tolist()))


def serial_model(payload, a0, nops, n):
    """The same facts by a walk over the bytes, one at a time: (ends, reg_end, T0, cnt, owner, row, halo_tokens, halo_bytes)."""
    p = bytes(np.asarray(payload, dtype=np.uint8).tobytes())
    vend = a0 + len(p)
    n_pieces = (vend + PIECE - 1) // PIECE if p else 0
    T0, cnt = [0] * n_pieces, [0] * n_pieces
    ends, owner, row, halo, halo_bytes = [], [], [], [0] * n_pieces, [0] * n_pieces
    seen, in_piece = 0, {}
    for off, byte in enumerate(p):
        if byte & 0x80:
            continue
        pc = (off + a0) // PIECE
        cnt[pc] += 1
        for later in range(pc + 1, n_pieces):
            T0[later] += 1
        if seen < n * nops:
            ends.append(off)
            if seen % nops == 0:
                owner.append(pc)
                row.append(in_piece.get(pc, 0) // 64)
                in_piece[pc] = in_piece.get(pc, 0) + 1
                halo[pc], halo_bytes[pc] = 0, 0
            elif pc != owner[-1]:
                halo[owner[-1]] += 1
            if seen % nops == nops - 1:      # the point's last byte: how far behind its owner's last byte
                halo_bytes[owner[-1]] = max(0, off + a0 - ((owner[-1] + 1) * PIECE - 1))
            seen += 1
    return ends, (ends[-1] + 1 if ends else 0), T0, cnt, owner, row, halo, halo_bytes


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


def chunk_points(n):
    return [CHUNK] * ((n - 1) // CHUNK) + [n - (n - 1) // CHUNK * CHUNK]


def models(streams, ns, a0, nops):
    """One Model per chunk of a batch whose streams lie back to back, the first payload at residue a0."""
    out, base = [], a0 - 4
    for stream, n in zip(streams, ns):
        for (off, payload), k in zip(split_chunks(stream), chunk_points(n)):
            out.append(Model(payload, (base + off) % 16, nops, k))
        base += len(stream)
    return out


# ---------------------------------------------------------------------------------------------------------------------
class Row:
    """build(a0) -> [(token codes, signs or None)] per cloud of the batch (one cloud unless the row says otherwise); ints(n) -> the
    integer columns of a cloud of n points. pred(M, a0) with M = models(...). a0s: the residues the row is built for (test_decode
    uses the first). stats / reg_end: HANDBACK rows only -- what the redo route reports."""

    def __init__(self, name, family, schema, build, pred, a0s=(4,), modes=None, ints=None, handback=False, reports=None):
        self.name, self.family, self.schema, self.build, self.pred, self.a0s = name, family, schema, build, pred, tuple(a0s)
        self.fields, self.step = SCHEMAS[schema]
        self.nops = nops_of(schema)
        self.modes, self.ints, self.handback = modes, ints, handback
        self.reports = reports        # HANDBACK rows: (decode_stats(), what reg_end is, sec_done or None) of the call
        self.base = None              # pinned(): the row whose token stream this one carries
        self.sections = bool(int_fields(schema))

    def info(self, n):
        return cases.make_info(self.fields, self.step, n)

    def clouds(self, a0):
        """[(n, cloud bytes)]"""
        out = []
        for codes, signs in self.build(a0):
            x = lanes_for(codes, self.nops, signs)
            n = len(x)
            cols = {f[0]: x[:, k] for k, f in enumerate(self.fields[:self.nops])}
            if self.sections:
                cols.update((self.ints or small_palettes)(self, n))
            out.append((n, cases.pack(self.info(n), cols, n)))
        return out

    def streams(self, oracle, a0):
        """([stream], [n], [cloud]) -- the oracle's bytes"""
        cl = self.clouds(a0)
        if self.modes is not None:
            st = [oracle.encode_stage1_continued(self.info(n), c, self.modes) for n, c in cl]
        else:
            st = [oracle.encode_stage1(self.info(n), c) for n, c in cl]
        return st, [n for n, _c in cl], [c for _n, c in cl]

    def models(self, streams, ns, a0):
        return models(streams, ns, a0, self.nops)

    def expect(self, M):
        """(decode_stats(), [reg_end per chunk]) of a decode call"""
        c = len(M)
        return (c, c if self.sections else 0, 0, 0), [m.reg_end for m in M]


PINNED = {3: "XYZ_U16", 4: "XYZW_U16"}
# one chunk with a Palette section, handed back: decode_varint_body<4, false> redoes the regular stream as above, then k_decode_tail's
# decode_sections_small_body decodes the Palette, counts the chunk under kStatFastSections and writes sec_done = 1 (stage1_decode.h);
# a chunk the point kernel keeps has its Palette folded into the point pass and sec_done = 2 (stage1_decode_wave.h, `folded`)
PINNED_REDO_REPORTS = ((1, 1, 0, 0), "regular end", 1)


def pinned(row):
    """The row's token stream, byte for byte, in front of one small Palette section (mode forced): XYZ / XYZW + UINT16. Without a
    section a chunk that k_decode_points_w hands back leaves the same decode_stats() and reg_end as one it keeps -- k_decode_varint
    redoes it under the same status word. With one, only the point kernel's fold writes sec_done == 2, so the twin shows whether the
    kernel kept the chunk. Rows that have sections are their own twin. The twin's predicate: its regular stream is the base row's
    payload (where the payload ends is the base row's own fact)."""
    if row.sections:
        return row
    def pred(M, a0, row=row):
        return all(m.reg_end < len(m.payload) and m.payload[m.reg_end] == 1 for m in M) and (row.handback or plain(M, a0))
    twin = Row(row.name, row.family, PINNED[row.nops], row.build, pred, row.a0s, modes=[1], handback=row.handback,
               reports=PINNED_REDO_REPORTS if row.handback else None)
    twin.base = row
    return twin


def carries_the_base_tokens(M, base_M):
    """every chunk's regular stream is the base row's payload"""
    return len(M) == len(base_M) and all(np.array_equal(m.payload[:m.reg_end], b.payload) and m.n == b.n for m, b in zip(M, base_M))


def small_palettes(row, n):
    i = np.arange(n, dtype=np.int64)
    return {f[0]: ((i * (3 + 2 * k) // 5) % (3 + k) * 257 + k).astype(cases._NP[f[2]]) for k, f in enumerate(int_fields(row.schema))}


def columns_not_palettes(row, n):
    """integer fields for the many-column variants, whose sections go to dense columns in front of the point kernel: ramps (DeltaRle),
    runs (Rle) and a small Palette"""
    i = np.arange(n, dtype=np.int64)
    vals = [i * 3 + 7, i // 37 * 5 % 11, i % 4 * 1000, i * 5 + 1, i // 50 % 7]
    return {f[0]: vals[k % 5].astype(cases._NP[f[2]]) for k, f in enumerate(int_fields(row.schema))}


def flaw_bait(row, n):
    """One integer field whose Palette table (first-occurrence order, raw little-endian values) begins with six (16 bit) or eight (32
    bit) bytes with the MSB set and then a 0x00 byte right behind an MSB-set one."""
    f, = int_fields(row.schema)
    table = [0x8080, 0x8181, 0x8282, 0x0080] if f[2] == F.UINT16 else [0x80808080, 0x81818181, 0x00808080, 0x7]
    return {f[0]: np.array(table, dtype=np.int64)[np.arange(n) % 4].astype(cases._NP[f[2]])}


# ---- predicates: pred(M, a0), M = one Model per chunk
def all_of(*preds):
    return lambda M, a0: all(p(M, a0) for p in preds)


def plain(M, a0):
    """what every row outside HANDBACK is: no token over 4 bytes, no 0x00 that ends a longer token, inside the regular stream"""
    return all(m.lens.max(initial=1) <= 4 and not np.any(m.markers & (m.lens > 1)) for m in M)


def token_at(V, length, o=None, marker=False, chunk=0):
    def pred(M, a0):
        m = M[chunk]
        i = np.nonzero(m.token_v() == V)[0]
        return len(i) == 1 and m.lens[i[0]] == length and (o is None or i[0] % m.nops == o) and bool(m.markers[i[0]]) == marker
    return pred


def pieces_at_least(k, chunk=0):
    return lambda M, a0: M[chunk].n_pieces >= k


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def _one(fn):
    """a builder of one cloud from a function a0 -> codes or (codes, signs)"""
    def build(a0):
        r = fn(a0)
        return [r if isinstance(r, tuple) else (r, None)]
    return build


def _unit_rows(T):
    # piece p = 1..16 holds a token of L bytes that ends at position p - 1 of lane 1's unit, of a middle unit and of lane 62's unit
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        for L in range(1, 5):
            def fn(a0, L=L, nops=nops):
                items = []
                for p in range(1, 17):
                    for lane in (1, 31, 62):
                        items.append(("pin", p * PIECE + (lane - 1) * UNIT + p - 1, L, None))
                return compose(a0, nops, items, more=40)

            def pred(M, a0, L=L):
                got = M[0].unit_positions()
                return all((place, pos, L) in got for place in (1, 0, UNITS) for pos in range(16)) and \
                    all(token_at(p * PIECE + (lane - 1) * UNIT + p - 1, L)(M, a0) for p in range(1, 17) for lane in (1, 31, 62))
            T.append(Row("unit_len%d_nops%d" % (L, nops), "unit", schema, _one(fn), all_of(plain, pred)))


def _boundary_rows(T):
    # piece edge p = 1, 2, ..: the (s, o) pairs one after the other, s = 0..L bytes of the token in front of the edge
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        for L in range(1, 5):
            pairs = [(s, o) for s in range(L + 1) for o in range(nops)]

            def fn(a0, L=L, nops=nops, pairs=pairs):
                return compose(a0, nops, [("pin", (k + 1) * PIECE - s + L - 1, L, o) for k, (s, o) in enumerate(pairs)], more=40)

            def pred(M, a0, L=L, nops=nops, pairs=pairs):
                got = M[0].boundary_splits()
                return all((L, s, o) in got for s, o in pairs) and \
                    all(token_at((k + 1) * PIECE - s + L - 1, L, o)(M, a0) for k, (s, o) in enumerate(pairs))
            T.append(Row("boundary_len%d_nops%d" % (L, nops), "boundary", schema, _one(fn), all_of(plain, pred)))


def _halo_rows(T):
    # the last point pieces 0 and 1 own: token nops - 1 - k ends on the piece's last byte, the k tokens behind it have 4 bytes each
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        for k in range(nops):
            def fn(a0, k=k, nops=nops):
                items = []
                for p in (1, 2):
                    items.append(("pin", p * PIECE - 1, 2, nops - 1 - k))
                    items.append(("run", [4] * k))
                return compose(a0, nops, items, more=60)

            def pred(M, a0, k=k):
                m = M[0]
                return m.halo_tokens[0] == k and m.halo_tokens[1] == k and m.halo_bytes[0] == 4 * k and m.halo_bytes[1] == 4 * k
            T.append(Row("halo_%d_tokens_nops%d" % (k, nops), "halo", schema, _one(fn), all_of(plain, pred)))


def _first_piece_rows(T):
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        for a0 in range(16):
            for L in range(1, 5):
                def fn(_a0, L=L, nops=nops):
                    return [L] + [1] * (nops - 1) + fill(40, 0, nops)
                T.append(Row("first_token_len%d_a0_%d_nops%d" % (L, a0, nops), "first_token", schema, _one(fn),
                             all_of(plain, lambda M, a0, L=L: M[0].lens[0] == L and M[0].a0 == a0 and M[0].ends[0] + a0 == a0 + L - 1),
                             a0s=(a0,)))
            for n in (1, 2, 5):
                def fn(_a0, n=n, nops=nops):
                    return [1 + (i * 3 + n) % 2 for i in range(n * nops)]
                T.append(Row("tiny_%d_points_a0_%d_nops%d" % (n, a0, nops), "tiny", schema, _one(fn),
                             all_of(plain, lambda M, a0, n=n: M[0].n == n and M[0].a0 == a0), a0s=(a0,)))
            size = 16 - a0        # the payload ends exactly on lane 1's last byte
            if size >= nops:
                def fn(_a0, size=size, nops=nops):
                    t = nops * ((size + 4 * nops - 1) // (4 * nops))     # the fewest whole points that can hold `size` bytes
                    return [1 + (size - t) // t + (1 if i < (size - t) % t else 0) for i in range(t)]
                T.append(Row("tiny_ends_with_lane_1_a0_%d_nops%d" % (a0, nops), "tiny", schema, _one(fn),
                             all_of(plain, lambda M, a0: M[0].vend == 16 and M[0].n_pieces == 1 and M[0].a0 == a0), a0s=(a0,)))


def _last_piece_rows(T):
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        for k in (1, 15, 16, 17, 991, 992):
            def fn(a0, k=k, nops=nops):
                return compose(a0, nops, [], total=2 * PIECE + k - a0)

            def pred(M, a0, k=k):
                m = M[0]
                return m.n_pieces == 3 and m.vend - PIECE * 2 == k and m.vend - PIECE == PIECE + k and m.reg_end == len(m.payload)
            T.append(Row("last_piece_%d_bytes_nops%d" % (k, nops), "last", schema, _one(fn), all_of(plain, pred)))


def _regend_rows(T):
    # The regular stream's last byte at v = 992 + k (k = 990, 991: the end of piece 1; 992, 993: the first bytes of piece 2; 1007: the
    # last byte of piece 1's halo unit, which is lane 1's unit of piece 2); a forced Palette section follows whose table bytes would be
    # flaws if they were tokens. The predicate looks at the 16 bytes behind the regular end, whichever unit they fall in. Which rows
    # reach `flaws &= keep`: the piece that closes the last point checks lanes 1..62 only, so at k = 992, 993 and 1007 the bait lies
    # in checked lanes of piece 2 and the mask must take it out; at k = 990 and 991 the closing piece is piece 1, the bait lies in
    # its halo (never checked) and in piece 2, which ends at `T0 >= target` before its flaws count -- those two rows guard the end
    # handling and the break, not the mask.
    for schema in ("XYZ_U16", "XYZ_U32"):
        for k, name in ((990, "990"), (991, "991"), (992, "0"), (993, "1"), (1007, "last_byte_of_the_halo_unit")):
            def fn(a0, k=k):
                return compose(a0, 3, [], total=PIECE + k + 1 - a0)

            def pred(M, a0, k=k):
                m = M[0]
                behind = m.payload[m.reg_end:m.reg_end + 16]
                msb = "".join("1" if b & 0x80 else "0" for b in behind)
                zero_behind_msb = any(behind[i] == 0 and behind[i - 1] & 0x80 for i in range(1, len(behind)))
                return m.reg_end - 1 + a0 == PIECE + k and m.reg_end < len(m.payload) and behind[0] == 1 and "11111" in msb and zero_behind_msb
            T.append(Row("regular_end_at_%s_%s" % (name, schema), "regend", schema, _one(fn), all_of(plain, pred), modes=[1], ints=flaw_bait))


def _nan_rows(T):
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        tag = "_nops%d" % nops

        # a marker at each token index, in points in the middle of piece 1
        def fn(a0, nops=nops):
            items = [("pin", PIECE + 300 + 40 * o, 0, o) for o in range(nops)]
            return compose(a0, nops, items, more=700)
        T.append(Row("nan_at_each_token_index" + tag, "nan", schema, _one(fn),
                     all_of(plain, *[token_at(PIECE + 300 + 40 * o, 1, o, marker=True) for o in range(nops)],
                            lambda M, a0, nops=nops: int(M[0].markers.sum()) == nops)))

        # first and last point piece 1 owns, and a halo token of piece 0's last point
        def fn(a0, nops=nops):
            items = [("pin", PIECE - 1, 1, 0), ("run", [0] + [1] * (nops - 2) + [0]), ("pin", 2 * PIECE - 1, 0, 0)]
            return compose(a0, nops, items, more=300)

        def pred(M, a0, nops=nops):
            m = M[0]
            f1, k1 = m.owned[1]
            mk = m.markers.reshape(m.n, nops)
            return m.halo_tokens[0] == nops - 1 and mk[f1 - 1, 1] and mk[f1].any() and mk[f1 + k1 - 1, 0] and int(mk.sum()) == 3 and \
                m.token_v()[(f1 + k1 - 1) * nops] == 2 * PIECE - 1
        T.append(Row("nan_in_first_and_last_owned_point_and_halo" + tag, "nan", schema, _one(fn), all_of(plain, pred)))

        # points 63 and 64 of piece 1: the two sides of a row boundary
        def fn(a0, nops=nops):
            body = [1] * (62 * nops) + [1] * (nops - 1) + [0] + [0] + [1] * (nops - 1) + [1] * (30 * nops)
            return compose(a0, nops, [("pin", PIECE, 1, 0), ("run", [1] * (nops - 1) + body)], more=500)

        def pred(M, a0, nops=nops):
            m = M[0]
            f1, _k = m.owned[1]
            mk = m.markers.reshape(m.n, nops)
            return m.token_v()[f1 * nops] == PIECE and mk[f1 + 63, nops - 1] and mk[f1 + 64, 0] and int(mk.sum()) == 2 and \
                m.row[f1 + 63] == 0 and m.row[f1 + 64] == 1
        T.append(Row("nan_in_points_63_and_64_of_a_piece" + tag, "nan", schema, _one(fn), all_of(plain, pred)))

        T.append(Row("nan_in_the_first_point" + tag, "nan", schema, _one(lambda a0, nops=nops: [0] + [2] * (nops - 1) + fill(1500, 0, nops)),
                     all_of(plain, lambda M, a0: M[0].markers[0] and int(M[0].markers.sum()) == 1)))

        def fn(a0, nops=nops):
            return compose(a0, nops, [("pin", PIECE + 200, 0, nops - 1), ("run", [2] * (nops - 1) + [0])], more=400)
        T.append(Row("nan_in_two_consecutive_points_of_a_lane" + tag, "nan", schema, _one(fn),
                     all_of(plain, token_at(PIECE + 200, 1, nops - 1, marker=True), token_at(PIECE + 200 + 2 * nops - 1, 1, nops - 1, marker=True))))

        def fn(a0, nops=nops):
            return compose(a0, nops, [("pin", PIECE + 100, 0, 0), ("run", [0] * (nops - 1)), ("pin", 2 * PIECE - 1, 0, 0), ("run", [0] * (nops - 1))],
                           more=300)
        T.append(Row("nan_whole_points" + tag, "nan", schema, _one(fn),
                     all_of(plain, lambda M, a0, nops=nops: int(M[0].markers.sum()) == 2 * nops and
                            M[0].markers.reshape(-1, nops).all(axis=1).sum() == 2 and M[0].halo_tokens[1] == nops - 1)))

        # every point of pieces 1 and 2 carries a marker, in lane j % nops; pieces 0 and 3 have none
        def fn(a0, nops=nops):
            head = compose(a0, nops, [("pin", PIECE - 1, 1, nops - 1)])
            body = []
            j = 0
            while sum(_blen(c) for c in body) < 2 * PIECE + 40:
                pt = [2, 1, 3, 1][:nops]
                pt[j % nops] = 0
                body += pt
                j += 1
            return head + body + fill(600, 0, nops)

        def pred(M, a0, nops=nops):
            m = M[0]
            mk = m.markers.reshape(m.n, nops).any(axis=1)
            (f1, k1), (f2, k2) = m.owned[1], m.owned[2]
            return mk[f1:f2 + k2].all() and not mk[:f1].any() and k1 > 128 and k2 > 128 and m.n_pieces >= 4
        T.append(Row("nan_in_every_point_of_two_pieces" + tag, "nan", schema, _one(fn), all_of(plain, pred)))

        # row 1 of piece 1 (its points 64..127) has a marker in every point, the rows around it none
        def fn(a0, nops=nops):
            body = [1] * (nops - 1) + [1] * (63 * nops)
            for j in range(64):
                pt = [1] * nops
                pt[j % nops] = 0
                body += pt
            return compose(a0, nops, [("pin", PIECE, 1, 0), ("run", body + [1] * (100 * nops))], more=600)

        def pred(M, a0, nops=nops):
            m = M[0]
            f1, k1 = m.owned[1]
            mk = m.markers.reshape(m.n, nops).any(axis=1)
            return k1 >= 192 and mk[f1 + 64:f1 + 128].all() and int(mk.sum()) == 64
        T.append(Row("nan_in_one_row_of_a_piece" + tag, "nan", schema, _one(fn), all_of(plain, pred)))


def _density_rows(T):
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        max_pts = (PIECE + nops - 1) // nops
        n1 = (3 * PIECE + 200) // nops
        T.append(Row("dense_1_byte_tokens_nops%d" % nops, "density", schema, _one(lambda a0, n1=n1, nops=nops: [1] * (n1 * nops)),
                     all_of(plain, pieces_at_least(4),
                            lambda M, a0, max_pts=max_pts: M[0].lens.max() == 1 and M[0].cnt[1] == PIECE and
                            max(k for _f, k in M[0].owned) == max_pts and M[0].row.max() == (max_pts - 1) // 64)))
        n4 = (3 * PIECE + 200) // (4 * nops)
        T.append(Row("dense_4_byte_tokens_nops%d" % nops, "density", schema, _one(lambda a0, n4=n4, nops=nops: [4] * (n4 * nops)),
                     all_of(plain, pieces_at_least(4),
                            lambda M, a0, nops=nops: M[0].lens.min() == 4 and M[0].cnt[1] == PIECE // 4 and
                            min(k for _f, k in M[0].owned[:3]) >= PIECE // (4 * nops) - 1)))


def _carry_rows(T):
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        # lane o climbs 17 + o steps of 2^20 ticks (beyond 2^24), then every token swings around that level
        def fn(a0, nops=nops):
            n = (4 * PIECE) // (3 * nops)
            codes = [4 if j < 17 + o else 3 for j in range(n) for o in range(nops)]
            signs = [1 if j < 17 + o else 0 for j in range(n) for o in range(nops)]
            return codes, signs

        def pred(M, a0, nops=nops):
            m = M[0]
            run = m.running()
            ok = m.n_pieces >= 4
            for pc in range(1, m.n_pieces):
                f, k = m.owned[pc]
                if f == 0:
                    return False
                front = run[f - 1]
                ok = ok and (front != 0).all() and len(set(front.tolist())) == nops and np.abs(front).max() > (1 << 24)
            return bool(ok)
        T.append(Row("carry_distinct_values_beyond_2_24_nops%d" % nops, "carry", schema, _one(fn), all_of(plain, pred)))
    # a piece that owns no point start. A point has at most 16 bytes, so only the payload's LAST piece can be one: the last point's
    # first token ends on the last byte of piece 2, its other three tokens (12 bytes) are all that piece 3 holds.
    def fn(a0):
        return compose(a0, 4, [("pin", 3 * PIECE - 1, 4, 0), ("run", [4, 4, 4])])

    def pred(M, a0):
        m = M[0]
        return m.n_pieces == 4 and m.owned[3][1] == 0 and m.cnt[3] == 3 and m.halo_tokens[2] == 3 and m.vend == 3 * PIECE + 12 and \
            m.T0[3] < m.n * 4 <= m.T0[3] + m.cnt[3]
    T.append(Row("carry_last_piece_owns_no_point_nops4", "carry", "XYZW", _one(fn), all_of(plain, pred)))


def _ring_rows(T):
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        def fn(a0, nops=nops):
            per = [1, 2, 1, 3, 2, 1, 4, 2, 1, 2, 3, 1]
            return [per[(g * 5 + g // 97) % 12] for g in range(CHUNK * nops)]
        T.append(Row("ring_full_chunk_nops%d" % nops, "ring", schema, _one(fn),
                     all_of(plain, lambda M, a0: M[0].n == CHUNK and M[0].n_pieces > 2 * RING + 1 and len(set(M[0].lens.tolist())) == 4)))

    # two chunks: the second payload lies at another residue than the first
    def fn(a0):
        first = [1, 1, 2, 1, 1, 1, 3, 1, 1] * (CHUNK // 3) + [1] * 6
        for i in range((7 - (sum(first) + 4)) % 16):    # the second payload: 7 residues further
            first[9 * i] = 2
        return first + fill(3 * PIECE, 0, 3)
    T.append(Row("ring_two_chunks_at_different_residues", "ring", "XYZ", _one(fn),
                 all_of(plain, lambda M, a0: len(M) == 2 and M[0].a0 == a0 and M[1].a0 != a0 and M[1].n_pieces >= 3)))

    # four clouds back to back, their payloads at four different residues
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        def build(a0, nops=nops):
            out, at = [], a0
            for k in range(4):
                assert at == (a0 + 5 * k) % 16
                size = 2 * PIECE + 100 * k
                size += ((a0 + 5 * (k + 1)) - (at + size + 4)) % 16
                out.append((compose(at, nops, [("pin", PIECE + k, 3, k % nops)], total=size), None))
                at = (at + size + 4) % 16
            return out
        T.append(Row("ring_ragged_batch_of_four_residues_nops%d" % nops, "ring", schema, build,
                     all_of(plain, lambda M, a0: len(M) == 4 and [m.a0 for m in M] == [(a0 + 5 * k) % 16 for k in range(4)] and
                            len({len(m.payload) for m in M}) == 4 and all(token_at(PIECE + k, 3, chunk=k)(M, a0) for k in range(4)))))


# one chunk, redone by decode_varint_body<4, false> behind the point kernel: see _handback_rows
REDO_REPORTS = ((1, 0, 0, 0), "payload size", None)


def _handback_rows(T):
    """Well-formed streams with one token of 5 bytes (a jump of 2^27 ticks). k_decode_points_w hands the chunk back (reg_end = kDecRedo,
    nothing counted); the schema has no sections, so k_decode_tail follows, whose first body is decode_varint_body<4, false>: dv_stream
    takes tokens of up to 7 bytes, decodes the chunk, writes reg_end = the offset behind the last token and counts the chunk under
    kStatFastRegular (stage1_decode.h, decode_varint_body). decode_general_body then finds nothing left (no V5 sections). Read from
    that code: decode_stats() == (chunks, 0, 0, 0) and reg_end == the payload's size -- the same figures the point kernel reports
    for a chunk it keeps; what tells the two apart is not visible through the hooks there are."""
    for nops, schema in ((3, "XYZ"), (4, "XYZW")):
        tag = "_nops%d" % nops
        for s in range(5):
            def fn(a0, s=s, nops=nops):
                return compose(a0, nops, [("pin", PIECE - s + 4, 5, None)], more=PIECE)
            T.append(Row("handback_5_bytes_%d_in_front_of_a_piece%s" % (s, tag), "handback", schema, _one(fn),
                         all_of(token_at(PIECE - s + 4, 5), lambda M, a0: int((M[0].lens == 5).sum()) == 1), handback=True, reports=REDO_REPORTS))
        T.append(Row("handback_5_bytes_first_token" + tag, "handback", schema, _one(lambda a0, nops=nops: [5] + [1] * (nops - 1) + fill(1200, 0, nops)),
                     lambda M, a0: M[0].lens[0] == 5 and int((M[0].lens == 5).sum()) == 1, handback=True, reports=REDO_REPORTS))
        T.append(Row("handback_5_bytes_last_token" + tag, "handback", schema, _one(lambda a0, nops=nops: fill(1200, 0, nops) + [1] * (nops - 1) + [5]),
                     lambda M, a0: M[0].lens[-1] == 5 and int((M[0].lens == 5).sum()) == 1 and M[0].reg_end == len(M[0].payload), handback=True, reports=REDO_REPORTS))


def _table():
    T = []
    for add in (_unit_rows, _boundary_rows, _halo_rows, _first_piece_rows, _last_piece_rows, _regend_rows, _nan_rows, _density_rows,
                _carry_rows, _ring_rows, _handback_rows):
        add(T)
    return T


ROWS = _table()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
HANDBACK = [r for r in ROWS if r.handback]
WELL_FORMED = [r for r in ROWS if not r.handback]
FAMILIES = ("unit", "boundary", "halo", "first_token", "tiny", "last", "regend", "nan", "density", "carry", "ring", "handback")

# one row of each family for 3 and 4 lanes (the section rows: 3 lanes only), and the two first-piece families whole
SUBSET = [BY_NAME[n] for n in (
    "unit_len3_nops3", "unit_len4_nops4", "boundary_len4_nops3", "boundary_len2_nops4", "halo_2_tokens_nops3", "halo_3_tokens_nops4",
    "last_piece_17_bytes_nops3", "last_piece_1_bytes_nops4", "regular_end_at_0_XYZ_U16", "regular_end_at_991_XYZ_U32",
    "nan_in_first_and_last_owned_point_and_halo_nops3", "nan_in_points_63_and_64_of_a_piece_nops4", "dense_1_byte_tokens_nops3",
    "dense_4_byte_tokens_nops4", "carry_distinct_values_beyond_2_24_nops3", "carry_last_piece_owns_no_point_nops4",
    "ring_ragged_batch_of_four_residues_nops3", "ring_ragged_batch_of_four_residues_nops4", "ring_two_chunks_at_different_residues")]
FIRST_PIECE = [r for r in ROWS if r.family in ("first_token", "tiny")]
