"""The value grid: clouds and hand-written streams aimed at the per-value arithmetic every codec route shares -- float -> tick ->
delta -> varint on the way in, tick -> float on the way out. No GPU, no library code. tests/test_value_grid_cases.py (CPU) proves
that every case is what its name says and pins it to the compiled reference; tests/test_gpu_value_grid.py runs the cases through
the encoders and decoders on the device. DESIGN.md section 4 ("The value grid") has the table in words.

A Case is one cloud of one layout at one resolution plus MARKS: facts about single tokens -- (point, lane) has this tick, this
reference (the tick of the point in front), this token length, and lies in a row of this TIER of the piece kernel
(stage1_fused.h): "fast" (float-domain formulas), "nan" (the NaN tier of the three-lane instantiations), "hard" (the integer
formulas) or "ovf" (a piece that overflows its LDS region and is rewritten by slow_piece). `Model` restates, in numpy, which tier a
row takes (from the kernel's comments: piece = 504 / 378 points, row = 63 points plus the point in front, zero in front of a
chunk, `any_nan` over the first two rows a wave loaded) and quantises with sweep_model._quantise. Values are ticks T at
resolutions where v = T * res and v * m are exact (0.5 and 1.0) unless a family says otherwise.

An ECase is a hand-written stage-1 stream ([u32 size], then zig-zag(+1) varints of chosen deltas, 0x00 for a NaN): running ticks no
encoder reaches from float input (above 2^24, int32 wrap-around, int64 values that round differently through double)."""
from __future__ import annotations

import numpy as np

import cases
import sweep_model as SM
import viz_grid_cases as VG

F = cases.F
CHUNK = 32768
ROW = 63                    # kRowPts
LIMIT = 1 << 21             # the float-domain path holds while every |rndne(v * m)| of the row is below this
PIECE = {3: 504, 4: 378}    # fused_piece_points
TIERS = ("fast", "nan", "hard", "ovf")

# layout -> ([(name, offset, type, lossy)], point step, the site the layout is named for)
_X = [("x", 0, F.FLOAT32, True), ("y", 4, F.FLOAT32, True), ("z", 8, F.FLOAT32, True)]
LAYOUTS = {
    "XYZ": (_X, 12, "piece kernel, 3 lanes (stage1_fused.h); k_decode_points_w"),
    "XYZI4": (_X + [("i", 12, F.FLOAT32, True)], 16, "piece kernel, 4 lanes; k_decode_points_w"),
    "XYZ_PAD_I": (_X + [("i", 16, F.FLOAT32, True)], 32, "piece kernel, fourth lane one dword further (l3 = 4)"),
    "XYZ_UNAL": ([("x", 1, F.FLOAT32, True), ("y", 5, F.FLOAT32, True), ("z", 9, F.FLOAT32, True)], 13, "piece kernel, unaligned loads"),
    "XYZ_F64": (_X + [("t", 16, F.FLOAT64, True)], 32, "piece kernel, TAIL op lossy FLOAT64 (quant_away_i64_f64)"),
    "XYZ_U16_F32": (_X + [("r", 12, F.UINT16, False), ("s", 16, F.FLOAT32, True)], 20, "piece kernel, TAIL op lossy FLOAT32 (quant_away_i64_f32)"),
    "FIVE": ([("abcde"[k], 4 * k, F.FLOAT32, True) for k in range(5)], 20, "generic kernel (stage1_kernels.hip): every lane scalar"),
    "LONE32": ([("a", 0, F.FLOAT32, True)], 4, "generic kernel, a lone lossy FLOAT32"),
    "LONE64": ([("a", 0, F.FLOAT64, True)], 8, "generic kernel, a lone lossy FLOAT64"),
    "COPY_F_COPY": ([("c0", 0, F.FLOAT32, False), ("a", 4, F.FLOAT32, True), ("c1", 8, F.FLOAT32, False)], 12,
                    "a lossy float between two copied fields: the stream / automaton decoders"),
    "WIDE": (_X + [("s", 12, F.FLOAT32, True), ("t", 16, F.FLOAT64, True)], 1040, "beyond the launch-argument plan (stage1_wide.h)"),
}
PIECE_LAYOUTS = ("XYZ", "XYZI4", "XYZ_PAD_I", "XYZ_UNAL", "XYZ_F64", "XYZ_U16_F32")
POINT_DECODER_LAYOUTS = ("XYZ", "XYZI4", "XYZ_PAD_I", "XYZ_UNAL")
TAIL_LAYOUTS = ("XYZ_F64", "XYZ_U16_F32")


def fields_of(layout, res):
    return [(nm, off, t, float(res) if lossy else None) for nm, off, t, lossy in LAYOUTS[layout][0]]


def info_of(layout, res, n):
    return cases.make_info(fields_of(layout, res), LAYOUTS[layout][1], n)


def lanes_of(layout):
    """[(field name, numpy dtype)] of the lossy float fields, in schema order"""
    return [(nm, "<f8" if t == F.FLOAT64 else "<f4") for nm, _off, t, lossy in LAYOUTS[layout][0] if lossy]


def kinds_of(layout):
    """sweep_model's kind per lane: FLOATN for the 3 or 4 leading lossy FLOAT32 fields, SCALAR32 / SCALAR64 otherwise"""
    k = SM.field_kinds(info_of(layout, 1.0, 1))
    return [k[i] for i, f in enumerate(LAYOUTS[layout][0]) if f[3]]


def n_floatn(layout):
    return sum(1 for k in kinds_of(layout) if k == SM.FLOATN)


def other_columns(layout, n):
    """the fields that carry no tick: a small Palette for an integer field, any bytes (MSBs and zero bytes included) for a copied one"""
    i = np.arange(n, dtype=np.int64)
    out = {}
    for k, (nm, _off, t, lossy) in enumerate(LAYOUTS[layout][0]):
        if lossy:
            continue
        if t == F.FLOAT32:
            out[nm] = ((i * 2654435761 + k * 40503) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
        else:
            out[nm] = (i % 7 * 3).astype(cases._NP[t])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# tokens and tiers, in numpy
# ---------------------------------------------------------------------------------------------------------------------
def lane_tokens(kind, v, res):
    """(q, ref, d, length, nan) per point of one lane: q from sweep_model._quantise, the reference 0 at a chunk start and behind a
    NaN, the delta with the lane's wrap-around, the token's bytes. All int64; d of a FLOATN lane is the sign-extended int32."""
    r32 = np.float32(res)
    nan = np.isnan(v)
    q = SM._quantise(kind, v, r32)
    ref = np.zeros(len(v), dtype=np.int64)
    ref[1:] = np.where(nan[:-1], 0, q[:-1])
    ref[::CHUNK] = 0
    with np.errstate(all="ignore"):
        if kind == SM.FLOATN:
            d = (q.astype(np.int32).view(np.uint32) - ref.astype(np.int32).view(np.uint32)).view(np.int32).astype(np.int64)
            u = ((d << 1) ^ (d >> 63)) + 1                       # at most 2^32: exact in int64
            length = SM._groups7(u.astype(np.uint64)).astype(np.int64)
        else:
            d = (q.view(np.uint64) - ref.view(np.uint64)).view(np.int64)
            u = ((d.view(np.uint64) << np.uint64(1)) ^ (d >> np.int64(63)).view(np.uint64)) + np.uint64(1)
            length = np.where(u == 0, 1, SM._groups7(np.where(u == 0, np.uint64(1), u)).astype(np.int64))
    return q, ref, d, np.where(nan, 1, length), nan


def row_tiers(vals, res, nl, small):
    """Per point: the tier of its row in the piece kernel. vals: float32 [n, nl], the FloatN lanes. small: the instantiation without a
    TAIL op, whose region holds 3 bytes per token (fused_region_cap_small)."""
    n = len(vals)
    piece = PIECE[nl]
    with np.errstate(all="ignore"):
        rr = np.rint((vals * (np.float32(1.0) / np.float32(res))).astype(np.float32))
        nan_pt = np.isnan(vals).any(axis=1)
        rare_pt = (~(np.abs(rr) < np.float32(LIMIT))).any(axis=1)                        # NaN, Inf, 2^21 ticks and more
        hard_pt = (~(np.abs(np.where(np.isnan(vals), np.float32(0), rr)) < np.float32(LIMIT))).any(axis=1)
    nbytes = np.zeros(n, dtype=np.int64)
    for k in range(nl):
        nbytes += lane_tokens(SM.FLOATN, vals[:, k], res)[3]
    cap = (piece * 3 * nl + 15) & ~15
    tier = np.empty(n, dtype="<U4")
    for c0 in range(0, n, CHUNK):
        nc = min(CHUNK, n - c0)
        for first in range(0, nc, piece):
            npc = min(piece, nc - first)
            g0 = c0 + first
            # the two rows a wave loads first: lane 0 of row 0 is the point in front of the piece (none at a chunk start)
            nan_tier = nl == 3 and bool(nan_pt[g0 - (1 if first else 0):g0 + min(npc, 2 * ROW)].any())
            ovf = small and int(nbytes[g0:g0 + npc].sum()) > cap
            for r0 in range(0, npc, ROW):
                r1 = min(r0 + ROW, npc)
                lanes = list(range(g0 + r0, g0 + r1))
                if r0 or first:
                    lanes.append(g0 + r0 - 1)        # lane 0: the point in front (at a chunk start: zeros)
                if r0 + ROW > npc:
                    lanes.append(g0)                 # lanes behind the piece's last point hold its first point
                rare, hard = bool(rare_pt[lanes].any()), bool(hard_pt[lanes].any())
                tier[g0 + r0:g0 + r1] = "ovf" if ovf else "fast" if not rare else "nan" if nan_tier and not hard else "hard"
    return tier


class Model:
    """Of one Case: per lane q, ref, d, length, nan; per point the tier (piece layouts only)."""

    def __init__(self, case):
        self.kinds = kinds_of(case.layout)
        self.lanes = [lane_tokens(k, v, case.res) for k, v in zip(self.kinds, case.v)]
        nl = n_floatn(case.layout)
        self.tier = None
        if case.layout in PIECE_LAYOUTS:
            vals = np.stack([case.v[k] for k in range(nl)], axis=1).astype(np.float32)
            self.tier = row_tiers(vals, case.res, nl, small=case.layout not in TAIL_LAYOUTS)

    def regular_bytes(self):
        return int(sum(int(ln[3].sum()) for ln in self.lanes))


class Mark:
    def __init__(self, point, lane, tier=None, length=None, q=None, ref=None, d=None, tag=None):
        self.point, self.lane, self.tier, self.length, self.q, self.ref, self.d, self.tag = point, lane, tier, length, q, ref, d, tag

    def holds(self, m):
        q, ref, d, length, _nan = (a[self.point] for a in m.lanes[self.lane])
        return (self.tier is None or m.tier is None or m.tier[self.point] == self.tier) and (self.length is None or length == self.length) and \
            (self.q is None or q == self.q) and (self.ref is None or ref == self.ref) and (self.d is None or d == self.d)

    def __repr__(self):
        return "Mark(point %d lane %d tier %s length %s q %s ref %s d %s %s)" % (self.point, self.lane, self.tier, self.length, self.q, self.ref,
                                                                                self.d, self.tag)


class Case:
    def __init__(self, name, family, layout, res, n):
        self.name, self.family, self.layout, self.res, self.n = name, family, layout, res, n
        self.v = [np.zeros(n, dtype=dt) for _nm, dt in lanes_of(layout)]
        self.marks = []

    def tick(self, lane, point, T):
        x = self.v[lane].dtype.type(T * self.res)
        assert float(x) / self.res == T, (T, self.res)       # exactly representable
        self.v[lane][point] = x

    def put(self, lane, point, value):
        self.v[lane][point] = value

    def mark(self, *a, **k):
        self.marks.append(Mark(*a, **k))

    def info(self):
        return info_of(self.layout, self.res, self.n)

    def cloud(self):
        cols = {nm: self.v[k] for k, (nm, _dt) in enumerate(lanes_of(self.layout))}
        cols.update(other_columns(self.layout, self.n))
        return cases.pack(self.info(), cols, self.n)

    def pred(self, model=None):
        m = model or Model(self)
        return [k for k in self.marks if not k.holds(m)]


def zz1_len(d):
    """bytes of the varint of zigzag(d) + 1, d a Python int of 32 bits"""
    u = ((d << 1) ^ (d >> 63)) + 1
    n = 1
    while u >> (7 * n):
        n += 1
    return n


def tier_of_ticks(*ticks):
    return "hard" if any(abs(t) >= LIMIT for t in ticks) else "fast"


# ---------------------------------------------------------------------------------------------------------------------
# family A: the 2^21 switch
# ---------------------------------------------------------------------------------------------------------------------
A_TICKS = [s * t for t in (LIMIT - 2, LIMIT - 1, LIMIT, LIMIT + 1, 2 * LIMIT - 1) for s in (1, -1)]
A_INDEXES = (0, 1, 62, 63, 64, 503, 504, 505, 377, 378, 379, 32767, 32768)
_A_FRONT_ONLY = (61, 376, 502, 32766)        # so that every listed index also has the tick in the point in front
A_N = CHUNK + 300
RES = 0.5


def _tick_name(t):
    return ("m" if t < 0 else "p") + str(abs(t))


def family_a(layout):
    """Per tick and lane two clouds: the placements at even and at odd indexes, so that each is a point's own value (zeros around it)
    and the value of the point in front of the next one. At index 32768 the reference is 0 whatever stands in front."""
    nl = n_floatn(layout)
    out = []
    for T in A_TICKS:
        tier = tier_of_ticks(T)
        for lane in range(nl):
            for parity in (0, 1):
                c = Case("A/%s/%s/lane%d/%s" % (layout, _tick_name(T), lane, ("even", "odd")[parity]), "A", layout, RES, A_N)
                placed = [i for i in A_INDEXES + _A_FRONT_ONLY if i % 2 == parity]
                for i in placed:
                    c.tick(lane, i, T)
                for i in placed:
                    ref = 0 if i % CHUNK == 0 or i - 1 not in placed else T
                    if i in A_INDEXES:
                        c.mark(i, lane, tier=tier, q=T, ref=ref, length=zz1_len(T - ref), tag=("own", T, i, lane))
                    if i + 1 in A_INDEXES and i + 1 not in placed:
                        if (i + 1) % CHUNK == 0:     # the chunk edge: reference 0, a one-byte token in a row that holds no big value
                            c.mark(i + 1, lane, tier="fast", q=0, ref=0, length=1, tag=("front", T, i + 1, lane))
                        else:
                            c.mark(i + 1, lane, tier=tier, q=0, ref=T, length=zz1_len(-T), tag=("front", T, i + 1, lane))
                out.append(c)
    # alternating-sign runs: |d| = 2^22 - 2 is the largest delta the fast path may see; 2^21 and 2^22 - 1 are hard rows
    for T in (LIMIT - 1, LIMIT, 2 * LIMIT - 1):
        for lane in range(nl):
            c = Case("A/%s/alternating_%d/lane%d" % (layout, T, lane), "A", layout, RES, 1100)
            for i in range(10, 210):
                c.tick(lane, i, T if i % 2 == 0 else -T)
            for i in (11, 12, 62, 63, 64, 100, 101, 209):
                s = 1 if i % 2 == 0 else -1
                c.mark(i, lane, tier=tier_of_ticks(T), q=s * T, ref=-s * T, d=2 * s * T, length=zz1_len(2 * s * T), tag=("alt", T))
            out.append(c)
    # a run in every lane over a whole piece: 4 bytes per token where the small region holds 3 -- slow_piece writes the piece
    if layout not in TAIL_LAYOUTS:
        T, p = LIMIT - 1, PIECE[nl]
        c = Case("A/%s/alternating_overflows_the_region" % layout, "A", layout, RES, 3 * p + 17)
        for lane in range(nl):
            for i in range(p, 2 * p):
                c.tick(lane, i, T if (i + lane) % 2 == 0 else -T)
        for lane in range(nl):
            for i in (p, p + 1, p + 62, p + 63, 2 * p - 1):
                s = 1 if (i + lane) % 2 == 0 else -1
                c.mark(i, lane, tier="ovf", q=s * T, length=4, tag=("ovf", T))
        c.mark(p - 1, 0, tier="fast", length=1)
        c.mark(2 * p + 63, 0, tier="fast", length=1)          # (row 0 of the next piece has the run's last point in front)
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family B: token lengths in each tier
# ---------------------------------------------------------------------------------------------------------------------
def b_deltas(hard):
    """u = zigzag(d) + 1 in {2^(7L) - 2, 2^(7L) - 1, 2^(7L), 2^(7L) + 1}: both sides of each length threshold, both signs. The float
    tiers take the deltas whose two ticks stay below 2^21."""
    out = []
    for L in (1, 2, 3, 4):
        h = 1 << (7 * L - 1)
        for d in (h - 1, -(h - 1), -h, h):
            a = -(d // 2)
            if float(np.float32(a)) != a or float(np.float32(a + d)) != a + d:     # 2^27 - 1 from -2^26 would need 26 bits: end at +-15
                a = (15 if d > 0 else -15) - d
            if hard or (abs(a) < LIMIT and abs(a + d) < LIMIT):
                out.append((d, a, a + d))
    return out


B_CONTEXTS = {3: ("fast", "nan", "late_nan", "inf"), 4: ("fast", "nan4", "inf")}
# context -> (row of piece 1 that holds the tokens, what stands in another lane of that row, the tier)
_B_CTX = {"fast": (1, None, "fast"), "nan": (1, np.nan, "nan"), "late_nan": (3, np.nan, "hard"), "inf": (1, np.inf, "hard"),
          "nan4": (1, np.nan, "hard")}


def family_b(layout):
    nl = n_floatn(layout)
    p = PIECE[nl]
    out = []
    for ctx in B_CONTEXTS[nl]:
        r, special, tier = _B_CTX[ctx]
        deltas = b_deltas(tier == "hard")
        assert len(deltas) <= 16
        for lane in range(nl):
            c = Case("B/%s/%s/lane%d" % (layout, ctx, lane), "B", layout, RES, 2 * p + 100)
            base = p + ROW * r
            for j, (d, a, b) in enumerate(deltas):
                s = base + 2 + 3 * j
                c.tick(lane, s - 1, a)
                c.tick(lane, s, b)
                c.mark(s, lane, tier=tier, q=b, ref=a, d=d, length=zz1_len(d), tag=("len", tier, zz1_len(d), 1 if d > 0 else -1))
            if special is not None:
                c.put((lane + 1) % nl, base + 55, special)
            c.mark(base - 2, lane, tier="fast", length=1)
            out.append(c)
    # a NaN as the point in front: the reference is 0; two NaNs in a row; NaN in lanes 0, 1, 62 and 63 of a row
    nan_tier = "nan" if nl == 3 else "hard"
    for lane in range(nl):
        c = Case("B/%s/nan_in_front/lane%d" % (layout, lane), "B", layout, RES, 2 * p + 100)
        s = p + 5
        for j, b in enumerate((63, 64, -64, 8191, 8192, -8192, (1 << 20) - 1, 1 << 20, -(1 << 20))):
            c.put(lane, s + 4 * j, np.nan)
            c.tick(lane, s + 4 * j + 1, b)
            c.mark(s + 4 * j + 1, lane, tier=nan_tier, q=b, ref=0, d=b, length=zz1_len(b), tag=("len", nan_tier, zz1_len(b), 1 if b > 0 else -1))
        c.put(lane, s + 50, np.nan)
        c.put(lane, s + 51, np.nan)
        c.tick(lane, s + 52, -8192)
        c.mark(s + 51, lane, tier=nan_tier, length=1)
        c.mark(s + 52, lane, tier=nan_tier, q=-8192, ref=0, length=3)
        out.append(c)
        c = Case("B/%s/nan_at_the_row_edges/lane%d" % (layout, lane), "B", layout, RES, 2 * p + 100)
        for r in (1, 3):         # (3 lanes: row 3 is not seen by any_nan -- row 1's NaN has chosen the tier for the piece)
            e = p + ROW * r      # lane 1 of row r; e - 1 is lane 63 of the row before and lane 0 of row r
            for i in (e - 1, e, e + 61, e + 62):
                c.put(lane, i, np.nan)
            c.tick(lane, e + 1, 64)
            c.tick(lane, e + 63, 64)
            c.mark(e, lane, tier=nan_tier, length=1)
            c.mark(e + 1, lane, tier=nan_tier, q=64, ref=0, length=2)
            c.mark(e + 62, lane, tier=nan_tier, length=1)
            c.mark(e + 63, lane, tier=nan_tier, q=64, ref=0, length=2)    # lane 1 of the next row: the NaN is its lane 0
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family C: rounding
# ---------------------------------------------------------------------------------------------------------------------
def _rne(k):       # k + 0.5 -> the even neighbour
    return k if k % 2 == 0 else k + 1


def family_c(layout):
    kinds = kinds_of(layout)
    out = []
    # m = 2: v = +-(k + 0.25) and +-(k + 0.75), the products the ties 2k + 0.5 and 2k + 1.5. FloatN lanes: half to even (2k, 2k + 2);
    # scalar lanes: half away from zero (2k + 1, 2k + 2)
    c = Case("C/%s/ties_at_m_2" % layout, "C", layout, 0.5, 200)
    for lane, kind in enumerate(kinds):
        for k in range(5):
            for j, (s, frac) in enumerate(((1, 0.25), (-1, 0.25), (1, 0.75), (-1, 0.75))):
                i = 10 + 8 * k + 2 * j + 60 * (lane % 2)
                c.put(lane, i, s * (k + frac))
                want = 2 * k + 2 if frac == 0.75 else 2 * k if kind == SM.FLOATN else 2 * k + 1
                c.mark(i, lane, q=s * want, ref=0, tier="fast", tag=("tie", kind))
    out.append(c)
    # res 1.0: the largest float32 below 0.5; odd integers in [2^23, 2^24]; -0.0 and a product that rounds to -0.0 in front of a
    # threshold token; a subnormal input (its product is subnormal too); 2^52 + 1 in a FLOAT64 lane
    c = Case("C/%s/edges_at_m_1" % layout, "C", layout, 1.0, 300)
    for lane, kind in enumerate(kinds):
        o = 5 + 97 * (lane % 3)
        below_half = np.nextafter(np.float32(0.5), np.float32(0)) if kind != SM.SCALAR64 else np.nextafter(0.5, 0.0)
        for j, (val, q) in enumerate(((below_half, 0), (-below_half, 0))):
            c.put(lane, o + 2 * j, val)
            c.mark(o + 2 * j, lane, q=q, ref=0, tier="fast", tag=("edge", kind))
        for j, (val, nxt) in enumerate(((-0.0, 63), (-0.0, 64), (-0.25, 63), (-0.25, -64), (1e-42, 64), (-1e-42, 8192))):
            i = o + 20 + 3 * j
            c.put(lane, i, val)
            c.put(lane, i + 1, nxt)
            c.mark(i, lane, q=0, length=1, tier="fast")
            c.mark(i + 1, lane, q=nxt, ref=0, d=nxt, length=zz1_len(nxt), tier="fast", tag=("after_zero", kind))
        if kind == SM.SCALAR64:
            c.put(lane, o + 50, float((1 << 52) + 1))
            c.mark(o + 50, lane, q=(1 << 52) + 1, ref=0, tag=("edge", kind))
            c.put(lane, o + 52, (1 << 51) + 0.5)             # a tie of the double product: away from zero
            c.mark(o + 52, lane, q=(1 << 51) + 1, ref=0, tag=("tie", kind))
    out.append(c)
    c = Case("C/%s/odd_integers_at_m_1" % layout, "C", layout, 1.0, 300)       # (FloatN lanes: hard rows)
    for lane, kind in enumerate(kinds):
        o = 5 + 97 * (lane % 3)
        for j, q in enumerate(((1 << 23) + 1, -(1 << 24) + 1, 1 << 24, (1 << 23) + 3, -(1 << 23) - 1)):
            c.put(lane, o + 2 * j, q)
            c.mark(o + 2 * j, lane, q=q, ref=0, tier="hard", tag=("odd", kind))
    out.append(c)
    # m = float32(1) / float32(res) for res 0.001 and 0.37: float32 neighbours whose float32 product is exactly k + 0.5 while the real
    # product is not (viz_grid_cases.float32_only_ties). The reverse -- a real product of exactly k + 0.5 that float32 moves off the
    # tie -- has no member: below 2^23 every k + 0.5 is a float32, so the float32 product of such a pair IS the tie.
    for res in (0.001, 0.37):
        v, t = VG.float32_only_ties(res, 20000)
        pick = np.concatenate([np.arange(0, min(40, len(v))), np.arange(max(0, len(v) - 40), len(v))]) if len(v) else np.zeros(0, int)
        c = Case("C/%s/float32_only_ties_at_%s" % (layout, res), "C", layout, res, 2 * len(pick) + 20)
        for lane, kind in enumerate(kinds):
            if kind == SM.SCALAR64:
                continue
            same_m = np.float32(1.0 / np.float64(np.float32(res))) == np.float32(1.0) / np.float32(res)
            for j, g in enumerate(pick):
                s = -1 if (j + lane) % 2 else 1
                c.put(lane, 10 + 2 * j, s * v[g])
                k = int(np.floor(t[g]))
                if kind == SM.FLOATN:
                    c.mark(10 + 2 * j, lane, q=s * _rne(k), ref=0, tier="fast", tag=("f32tie", res))
                elif same_m:
                    c.mark(10 + 2 * j, lane, q=s * (k + 1), ref=0, tag=("f32tie", res))
        c.n_ties = len(pick)
        if c.marks:          # (a layout of doubles alone has no float32 product)
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# family D: range
# ---------------------------------------------------------------------------------------------------------------------
I32_MIN, I64_MIN = -(1 << 31), -(1 << 63)


def family_d(layout):
    kinds = kinds_of(layout)
    c = Case("D/%s/range" % layout, "D", layout, 1.0, 400)
    nan, inf = np.nan, np.inf
    for lane, kind in enumerate(kinds):
        o = 3 + 130 * (lane % 3) + (lane // 3) * 60
        if kind == SM.FLOATN:
            top = 2147483520.0                           # 2^31 - 128, the largest float32 product inside the range
            seq = [(top, 2147483520, 5), (2147483648.0, I32_MIN, 2),      # the delta wraps in int32: 128, a 2-byte token
                   (0.0, 0, 5), (2147483648.0, I32_MIN, 5),               # d = INT32_MIN exactly: zigzag 0xffffffff
                   (-2147483648.0, I32_MIN, 1), (-2147483904.0, I32_MIN, 1), (0.0, 0, 5),
                   (inf, I32_MIN, 5), (inf, I32_MIN, 1), (nan, None, 1), (inf, I32_MIN, 5), (-inf, I32_MIN, 1), (nan, None, 1), (nan, None, 1),
                   (-top, -2147483520, 5), (top, 2147483520, 2),          # d = 2^32 - 256 wraps to -256: a 2-byte token
                   (0.0, 0, 5), (3.0e38, I32_MIN, 5), (-3.0e38, I32_MIN, 1), (0.0, 0, 5)]
        else:
            f32 = kind == SM.SCALAR32
            top = 9223371487098961920.0 if f32 else 9223372036854774784.0    # the largest float32 / double below 2^63
            seq = [(9223372036854775808.0, I64_MIN, 1), (nan, None, 1),       # the sentinel from reference 0: the one byte 0x00
                   (-9223372036854775808.0, I64_MIN, 1), (nan, None, 1), (3.0e38, I64_MIN, 1), (inf, I64_MIN, 1), (-inf, I64_MIN, 1), (nan, None, 1),
                   (top, int(top), 10), (0.0, 0, 10), (-top, -int(top), 10), (0.0, 0, 10),
                   (4611686018427387904.0, 1 << 62, 10), (0.0, 0, 10), (-4611686018427387904.0, -(1 << 62), 10), (0.0, 0, 10),
                   (2147483648.0, 1 << 31, 5), (nan, None, 1), (nan, None, 1), (-2147483904.0, -2147483904, 5)]
        for j, (val, q, length) in enumerate(seq):
            c.put(lane, o + j, val)
            c.mark(o + j, lane, q=q, length=length, tier="hard" if kind == SM.FLOATN else None, tag=("range", kind, j))
    out = [c]
    c = Case("D/%s/product_overflows" % layout, "D", layout, 0.5, 200)          # a finite v whose product is inf
    for lane, kind in enumerate(kinds):
        if kind == SM.SCALAR64:
            c.put(lane, 20, 1.0e308)
            c.mark(20, lane, q=I64_MIN, length=1)
            c.put(lane, 21, np.nan)
            continue
        i = 10 + 20 * (lane % 3)
        c.put(lane, i, 3.0e38)
        c.put(lane, i + 1, np.nan)
        c.put(lane, i + 2, -3.0e38)
        c.put(lane, i + 3, np.nan)
        sent, length = (I32_MIN, 5) if kind == SM.FLOATN else (I64_MIN, 1)
        c.mark(i, lane, q=sent, length=length, tier="hard" if kind == SM.FLOATN else None)
        c.mark(i + 2, lane, q=sent, ref=0, length=length)
    out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the encode grid
# ---------------------------------------------------------------------------------------------------------------------
_grid = {}


def family(fam, layout):
    key = (fam, layout)
    if key not in _grid:
        if fam in ("A", "B") and layout not in PIECE_LAYOUTS:
            _grid[key] = []
        else:
            _grid[key] = {"A": family_a, "B": family_b, "C": family_c, "D": family_d}[fam](layout)
    return _grid[key]


ENCODE_FAMILIES = ("A", "B", "C", "D")
GROUPS = [(fam, layout) for fam in ENCODE_FAMILIES for layout in LAYOUTS if not (fam in ("A", "B") and layout not in PIECE_LAYOUTS)]


def report_groups():
    """[(id, cases)] for the sweep and histogram reports: every cloud of A-D. Family A is cut by tick, so that no test holds more than
    the eight or so clouds of one tick (33 068 points each) and the numpy models stay within a second or two per test."""
    out = []
    for fam, layout in GROUPS:
        cs = family(fam, layout)
        if fam != "A":
            out.append((group_id((fam, layout)), cs))
            continue
        keys = []
        for c in cs:
            k = c.name.split("/")[2]
            if k not in keys:
                keys.append(k)
        for k in keys:
            out.append(("A-%s-%s" % (layout, k), [c for c in cs if c.name.split("/")[2] == k]))
    assert sum(len(cs) for _i, cs in out) == sum(len(family(*g)) for g in GROUPS)
    return out


def group_id(g):
    return "%s-%s" % g


# ---------------------------------------------------------------------------------------------------------------------
# family E: hand-written streams
# ---------------------------------------------------------------------------------------------------------------------
def varint(u):
    out = bytearray()
    while u > 0x7F:
        out.append((u & 0x7F) | 0x80)
        u >>= 7
    out.append(u)
    return bytes(out)


def token(d):
    """zig-zag(+1) varint of a delta; None = the NaN marker"""
    return b"\x00" if d is None else varint((((d << 1) ^ (d >> 63)) & ((1 << 64) - 1)) + 1)


def write_stream(layout, points, sections=b""):
    """One chunk: [u32 size], then per point its fields in schema order -- a token per lossy float (the entries of the point's list),
    four raw bytes per copied FLOAT32 -- then the sections of the integer fields, which the caller supplies"""
    body = bytearray()
    for i, deltas in enumerate(points):
        it = iter(deltas)
        for k, (_nm, _off, t, lossy) in enumerate(LAYOUTS[layout][0]):
            if lossy:
                body += token(next(it))
            elif t == F.FLOAT32:
                body += int((i * 2654435761 + k * 40503) & 0xFFFFFFFF).to_bytes(4, "little")
    body += bytes(sections)
    return np.frombuffer(len(body).to_bytes(4, "little") + bytes(body), dtype=np.uint8).copy()


def sections_of(oracle, layout, res, n):
    """The sections the oracle writes behind the regular stream for the layout's integer columns (other_columns): its stream of a cloud
    whose floats are all 0.0 is n one-byte tokens 0x01 per lane, then the sections."""
    if all(lossy or t == F.FLOAT32 for _nm, _off, t, lossy in LAYOUTS[layout][0]):
        return b""
    assert n <= CHUNK
    c = Case("zeros", "E", layout, res, n)
    payload = oracle.encode_stage1(c.info(), c.cloud())[4:]
    k = n * len(lanes_of(layout))
    assert np.all(payload[:k] == 1) and len(payload) > k
    return payload[k:].tobytes()


E_TICKS32 = [s * t for t in ((1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6) for s in (1, -1)] + [(1 << 31) - 1, -(1 << 31)]
E_TICKS64 = [(1 << 40) + (1 << 16) + 1, (1 << 62) + (1 << 38) + 1, -((1 << 62) + (1 << 38) + 1), (1 << 63) - 1, (1 << 53) + 1, (1 << 53) + 3]
E_RESOLUTIONS = (1.0, 0.001, 0.37)
E_LAYOUTS = tuple(LAYOUTS)
E_HOP = (1 << 27) - 1  # the largest hop of an int32 lane: u = zigzag + 1 < 2^28, a 4-byte token
E_QUIET = 800          # points without a marker behind the first ticks: more than two pieces (992 bytes) of one-byte tokens
E_PAD = 400            # points with a marker in front of and behind the second ticks: more than a piece on either side


class ECase:
    """stream(oracle), n, and `reached`: {(tick, lane, marker state)}; marker state 1 = every point for more than a piece (992 bytes) around
    carries a NaN marker in another lane (one lane: in the points next to it), 0 = no marker within two pieces. wraps: {(lane, marker
    state)} where an int32 lane's running value went from 2^31 - 1 to -2^31 by d = +1 and back by d = -1. max_token32: the longest
    token of an int32 lane."""

    def __init__(self, layout, res, nan_lane, long_tokens=False):
        self.layout, self.res, self.nan_lane, self.long_tokens = layout, res, nan_lane, long_tokens
        self.name = "E/%s/res_%s/nan_lane%d%s" % (layout, res, nan_lane, "/long_tokens" if long_tokens else "")
        kinds = kinds_of(layout)
        nl = len(kinds)
        cur = [0] * nl
        pts, self.reached, self.wraps = [], set(), set()
        self.first_tick_point, self.tick_points = {}, {0: [], 1: []}

        def quiet(count, marker):
            for j in range(count):
                row = [0] * nl
                if marker:
                    if nl > 1:
                        row[nan_lane], cur[nan_lane] = None, 0
                    elif j % 2:
                        row[0], cur[0] = None, 0
                pts.append(row)

        def run(marker):
            """Every lane walks its own list of targets, one hop per point. An int32 lane hops by less than 2^27 ticks, so that no token
            has more than 4 bytes (k_decode_points_w hands a chunk with a longer one back to the serial redo); from 2^31 - 1 it steps
            over the edge by d = +1 (-2^31: the carry wraps), back by d = -1, and walks down again. long_tokens: one step per target."""
            lanes = [k for k in range(nl) if not (marker and nl > 1 and k == nan_lane)]
            todo = {}
            for k in lanes:
                if kinds[k] == SM.FLOATN:
                    todo[k] = [x for T in E_TICKS32[:-2] for x in (T, 0)] + [(1 << 31) - 1, "over", "back", 0]
                else:
                    todo[k] = [x for T in E_TICKS32 + E_TICKS64 for x in (T, 0)]
            while any(todo.values()):
                row = [0] * nl
                for k in lanes:
                    if not todo[k]:
                        continue
                    t = todo[k][0]
                    if t == "over" or t == "back":
                        assert cur[k] == ((1 << 31) - 1 if t == "over" else -(1 << 31))
                        row[k] = 1 if t == "over" else -1
                        cur[k] = -(1 << 31) if t == "over" else (1 << 31) - 1
                        if t == "over":
                            self.reached.add((-(1 << 31), k, marker))
                            self.wraps.add((k, marker))
                        todo[k].pop(0)
                        continue
                    d = t - cur[k]
                    if kinds[k] == SM.FLOATN and not long_tokens:
                        d = max(-E_HOP, min(E_HOP, d))
                    assert -(1 << 63) <= d < (1 << 63), (t, cur[k])     # no int64 wrap-around: undefined in the reference
                    row[k] = d
                    cur[k] += d
                    if cur[k] == t:
                        todo[k].pop(0)
                        if t != 0:
                            self.reached.add((t, k, marker))
                if marker and nl > 1:
                    row[nan_lane] = None
                self.tick_points[marker].append(len(pts))
                pts.append(row)
                if marker and nl == 1:
                    pts.append([None])
                    cur[0] = 0
                    if todo[0] and todo[0][0] == 0:
                        todo[0].pop(0)

        run(0)
        self.quiet_from = len(pts)
        quiet(E_QUIET, 0)
        self.marked_from = len(pts)
        quiet(E_PAD, 1)
        run(1)
        quiet(E_PAD, 1)
        self.points = pts
        self.n = len(pts)
        self._stream = None

    def stream(self, oracle):
        """(the oracle only supplies the sections of an integer field: sections_of)"""
        if self._stream is None:
            self._stream = write_stream(self.layout, self.points, sections_of(oracle, self.layout, self.res, self.n))
        return self._stream

    def info(self):
        return info_of(self.layout, self.res, self.n)


_e = []


def e_cases():
    if not _e:
        for layout in E_LAYOUTS:
            nl = len(kinds_of(layout))
            for res in E_RESOLUTIONS:
                for nan_lane in ((nl - 1, 0) if nl > 1 else (0,)):
                    _e.append(ECase(layout, res, nan_lane))
                if layout in POINT_DECODER_LAYOUTS:
                    # the same ticks reached in one step: tokens of 5 bytes. k_decode_points_w hands such a chunk back and
                    # decode_varint_body<4, false> in k_decode_tail redoes it (dv_stream, stage1_decode.h: `(float)(int32_t)cur`)
                    _e.append(ECase(layout, res, nl - 1, long_tokens=True))
    return _e
