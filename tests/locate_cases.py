"""The case table of tests/test_locate_model.py (CPU) and tests/test_gpu_locate.py: one-chunk clouds built from chosen token
lengths, so that a payload's size, the place of its section and the bytes around it are the builder's choice. Every row is
fixed -- literals and arithmetic on them, no search and no filter at test time; the numbers that needed one (FRONT_PART) were found
once with tests/locate_model.py -- and the CPU test proves that each row takes the branch its name says. DESIGN.md section 4 has the table in words.

A float lane at resolution 0.001: a difference of 0 steps is a 1-byte token (0x01), of 100 steps a 2-byte one, of 10 000 steps a
3-byte one; NaN is the marker byte 0x00 and resets the lane. An integer field in DeltaVarint mode: differences of 0 / 100 /
10 000 / 2^22 / 2^30 give tokens of 1 / 2 / 3 / 4 / 5 bytes.
"""
from __future__ import annotations

import numpy as np

import cases

F = cases.F
RES = 0.001
TILE = {4: 4 * 4096, 16: 16 * 4096}       # bytes a step of the DeltaVarint guess reads (NW * 64 threads * 64 bytes)
WINDOW = {4: 4 * 1024, 16: 16 * 1024}     # the payload's last bytes the DeltaRle guess searches
FILLERS = 64                              # clouds added to a case for NW = 4: more than 64 chunks in the call

_XYZ = [("x", 0, F.FLOAT32, RES), ("y", 4, F.FLOAT32, RES), ("z", 8, F.FLOAT32, RES)]
SCHEMAS = {
    "xyz_u16": (_XYZ + [("f0", 12, F.UINT16, None)], 16),
    "xyz_u32": (_XYZ + [("f0", 12, F.UINT32, None)], 16),
    "xyzi_u16": (_XYZ + [("i", 12, F.FLOAT32, RES), ("f0", 16, F.UINT16, None)], 18),
    "xyz_u16_u16": (_XYZ + [("f0", 12, F.UINT16, None), ("f1", 14, F.UINT16, None)], 16),
}
_STEPS = {1: 0, 2: 100, 3: 10_000, 4: 1 << 22, 5: 1 << 30}


def schema(name, n):
    fields, step = SCHEMAS[name]
    info = cases.make_info(fields, step, n)
    lanes = [f[0] for f in fields if f[2] == F.FLOAT32]
    ints = [(f[0], 2 if f[2] == F.UINT16 else 4) for f in fields if f[2] != F.FLOAT32]
    return info, lanes, ints


def _toggle_values(lengths):
    """Values whose differences (to the value in front, 0 in front of the first) are tokens of the given lengths: one toggle
    per length class, so the values stay small."""
    lengths = np.asarray(lengths)
    v = np.zeros(len(lengths), dtype=np.int64)
    for ln, mag in _STEPS.items():
        if ln != 1:
            v += (np.cumsum(lengths == ln) % 2) * mag
    return v


def lane_floats(n, two=0, three=0, first=1, nan_at=(), plus=()):
    """A float lane of n points: `two` 2-byte and then `three` 3-byte tokens from point `first` on (differences of +-100 and
    +-10 000 steps in turn), the (point, steps) differences of `plus`, markers at nan_at (a marker resets the lane to 0)."""
    d = np.zeros(n, dtype=np.int64)
    d[first:first + two] = 100 * (1 - 2 * (np.arange(two) % 2))
    d[first + two:first + two + three] = 10_000 * (1 - 2 * (np.arange(three) % 2))
    for p, steps in plus:
        d[p] = steps
    isnan = np.zeros(n, dtype=bool)
    isnan[list(nan_at)] = True
    d[isnan] = 0
    c = np.cumsum(d)
    last = np.maximum.accumulate(np.where(isnan, np.arange(n), -1))
    q = c - np.where(last >= 0, c[np.maximum(last, 0)], 0)
    f = (q.astype(np.float64) * RES).astype(np.float32)
    f[isnan] = np.nan
    return f


def field_values(spec, n, bpv):
    """The integer field of a case. spec: ("dv", [(count, token length), ...]) | ("ring", rings) | ("runs", run length, values)
    | ("noise", seed) | ("many", distinct values)."""
    kind = spec[0]
    if kind == "dv":
        lengths = np.concatenate([np.full(c, ln, dtype=np.int64) for c, ln in spec[1]])
        assert len(lengths) == n, (len(lengths), n)
        return _toggle_values(lengths)
    if kind == "ring":
        return np.arange(n, dtype=np.int64) % spec[1]
    if kind == "runs":
        vals = np.asarray(spec[2], dtype=np.int64)
        return vals[(np.arange(n) // spec[1]) % len(vals)]
    if kind == "noise":
        return np.random.RandomState(spec[1]).randint(0, 1 << (8 * bpv), n).astype(np.int64)
    if kind == "many":     # spec[1] distinct values whose bytes all have the MSB set; the last point takes the last of them
        k = np.arange(n, dtype=np.int64) % spec[1]
        k[-1] = spec[1] - 1
        return 0x8080 + (k % 128) + ((k // 128) << 8)
    raise ValueError(kind)


class Case:
    def __init__(self, name, schema_name, n, branch, modes, fields, right=True, x=(0, 0), nan=None, plus=None, size=None,
                 section=None, cols=1, sec_done=2, dv_chunks=0, split=(0,), note="", part_k=None, assemble=False):
        self.name, self.schema, self.n, self.branch, self.modes, self.fields = name, schema_name, n, branch, list(modes), fields
        self.right = right            # the branch's place is the plain token count's
        self.x = x                    # (2-byte tokens, 3-byte tokens) of lane x
        self.nan = nan or {}          # lane -> points with a marker
        self.plus = plus or {}        # lane -> (point, steps)
        self.size = size              # the payload's bytes (asserted by the CPU test), None: not pinned
        self.section = section        # the bytes of the sections (size - section = the regular stream), None: not pinned
        self.cols, self.sec_done, self.dv_chunks = cols, sec_done, dv_chunks   # what the model must derive
        self.split = split            # cldn_hip_debug_decode_split values the GPU test runs the case with
        self.note = note
        self.part_k = part_k          # front_part_*: the wave whose part begins at (or one byte in front of) the section
        self.assemble = assemble      # the section is big_palette_section(n), put behind the oracle's regular stream

    def build(self, oracle):
        """(info, cloud bytes, stream, payload of the one chunk). The cloud is what the oracle encoded; the decoders' reference is
        always the oracle's decode of `stream`."""
        info, lanes, ints = schema(self.schema, self.n)
        cols = {}
        for k, ln in enumerate(lanes):
            two, three = self.x if k == 0 else (0, 0)
            cols[ln] = lane_floats(self.n, two, three, nan_at=tuple(self.nan.get(ln, ())), plus=tuple(self.plus.get(ln, ())))
        for (name, bpv), spec in zip(ints, self.fields):
            cols[name] = field_values(spec, self.n, bpv).astype(np.uint16 if bpv == 2 else np.uint32)
        cloud = cases.pack(info, cols, self.n)
        stream = oracle.encode_stage1_continued(info, cloud, self.modes)
        size = int(np.frombuffer(stream[:4].tobytes(), "<u4")[0])
        assert size + 4 == len(stream), "one chunk"
        if self.assemble:
            ends = np.nonzero((stream[4:] & 0x80) == 0)[0]
            regular = stream[4:4 + int(ends[self.n * len(lanes) - 1]) + 1]
            payload = np.concatenate([regular, big_palette_section(self.n)])
            stream = np.concatenate([np.frombuffer(np.uint32(len(payload)).tobytes(), np.uint8), payload])
        return info, cloud, stream, stream[4:]


def filler(oracle, schema_name):
    """The small cloud that fills a call up to more than 64 chunks (k_locate_sections<4>, the chained launch)."""
    c = Case("filler", schema_name, 40, "front", [0] * len(schema(schema_name, 40)[2]),
             [("dv", [(40, 2)])] * len(schema(schema_name, 40)[2]))
    return c.build(oracle)


def _dv(n, **counts):
    """DeltaVarint token lengths of a field: b2=.. tokens of 2 bytes, b3, b4, b5; the rest 1 byte."""
    rows, left = [], n
    for ln in (5, 4, 3, 2):
        c = counts.get("b%d" % ln, 0)
        if c:
            rows.append((c, ln))
            left -= c
    return ("dv", [(left, 1)] + rows) if left else ("dv", rows)


def _marker(m):
    """Token number m (0-based) of a 3-lane regular stream as a marker: {lane: [point]}."""
    return {"xyz"[m % 3]: [m // 3]}


def _table():
    T = []
    for nw in (4, 16):
        t = TILE[nw]
        s = "nw%d_" % nw
        q = nw // 4                       # the NW = 16 cases are the NW = 4 ones with four times the points
        # ---- DeltaVarint guess, right. The regular stream has 3 n (4 n) bytes + one per 2-byte token + two per 3-byte token,
        # the section 1 + the token bytes; the mode byte lies at size - section
        n = 4000 * q
        sec = n + 1
        T.append(Case(s + "dv_size_tile_plus_15", "xyz_u16", n, "front", [0], [_dv(n)], x=(t + 15 - 3 * n - sec, 0), size=t + 15,
                      section=sec, dv_chunks=1, note="hi >= TILE + 16 fails by one byte: no tile is read"))
        T.append(Case(s + "dv_size_tile_plus_16", "xyz_u16", n, "dv_end", [0], [_dv(n)], x=(t + 16 - 3 * n - sec, 0), size=t + 16,
                      section=sec, dv_chunks=1, note="the smallest payload whose last tile is read"))
        # the wanted end in tile 1, 2, 3: 5-byte tokens of a 32-bit field make the section as long as wanted
        n = 8000 * q
        for tile_no, want in ((1, 0), (2, t + t // 2), (3, 2 * t + t // 8)):
            b5 = (want - n) // 4 if want else 0
            sec = n + 1 + 4 * b5
            assert (tile_no - 1) * t < sec <= tile_no * t and b5 <= n
            T.append(Case(s + "dv_tile%d" % tile_no, "xyz_u32", n, "dv_end", [0], [_dv(n, b5=b5)], x=(n - 1, 0),
                          size=4 * n - 1 + sec, section=sec, dv_chunks=1, note="`seen` carries over %d tiles" % (tile_no - 1)))
        # the wanted end at chosen bytes of a thread's 64 and of a 16-byte unit: section - 1 bytes lie behind it
        n = 5400 * q
        for what, rem in (("thread_first_byte", 63), ("thread_last_byte", 0), ("unit_first_byte", 47), ("unit_last_byte", 16)):
            b2 = (rem - n) % 64           # section - 1 = n + b2 = rem (mod 64)
            sec = n + 1 + b2
            T.append(Case(s + "dv_" + what, "xyz_u16", n, "dv_end", [0], [_dv(n, b2=b2)], x=(n - 1, 0), size=4 * n - 1 + sec,
                          section=sec, dv_chunks=1))
        b5 = (t - n - 1) // 4             # section = TILE exactly: the mode byte is the tile's lowest byte
        b2 = t - (n + 1 + 4 * b5)
        T.append(Case(s + "dv_tile_lowest_byte", "xyz_u32", n, "dv_end", [0], [_dv(n, b5=b5, b2=b2)], x=(n - 1, 0),
                      size=4 * n - 1 + t, section=t, dv_chunks=1))
        n = 6000 * q
        T.append(Case(s + "dv_standing_still", "xyz_u16", n, "dv_end", [0], [_dv(n, b3=n)], size=6 * n + 1, section=3 * n + 1,
                      dv_chunks=1, note="every regular token 1 byte: at == n * n_ops exactly"))
        n = 4000 * q
        T.append(Case(s + "dv_in_front_of_the_tiles", "xyz_u32", n, "front", [0], [_dv(n, b5=n)], size=8 * n + 1, section=5 * n + 1,
                      dv_chunks=1, note="one tile fits, the section is longer: the wanted end is never reached"))
        n = 5400 * q
        T.append(Case(s + "dv_4ops", "xyzi_u16", n, "dv_end", [0], [_dv(n, b2=n // 2)], x=(n - 1, 0), dv_chunks=1))
        # ---- DeltaVarint guess, refused. A one-run Rle section 02 01 00 00 00 91 91 <length> holds 6 token ends, so the
        # (n + 1)-th end from the back is token number 2 n + 5 of the regular stream
        rle = [("runs", n, [0x9191])]
        T.append(Case(s + "dv_refused_at_too_small", "xyz_u16", n, "front", [2], rle, nan=_marker(2 * n + 5), x=(300 * q, 0),
                      note="a marker, but too few bytes lie in front of it: at = 2 n + 5 + 300 q < 3 n"))
        T.append(Case(s + "dv_refused_no_mode_byte", "xyz_u16", n, "front", [2], rle, x=(0, n - 1),
                      note="the (n + 1)-th end from the back is a 0x01 of the regular stream, behind more than 3 n bytes"))
        T.append(Case(s + "dv_refused_not_closed", "xyz_u16", n, "front", [1], [("many", 1100)], x=(n - 1, 0),
                      note="a Palette of 1100 entries: beyond kFastPalEntries, and its last index byte has the MSB set"))
        # ---- DeltaVarint guess, wrong (a): the same marker behind 3-byte x tokens (at >= 3 n), another marker behind it:
        # k_section_dv_w hands the chunk back
        later = _marker(2 * n + 5)
        later.setdefault("z", []).append(n - 20)
        T.append(Case(s + "dv_wrong_markers_behind", "xyz_u16", n, "dv_end", [2], rle, right=False, nan=later, x=(0, n - 1),
                      cols=0, sec_done=1, split=(0, 1)))
        # ---- DeltaRle from the end
        T.append(Case(s + "drle_ring", "xyzi_u16", n, "drle_end", [3], [("ring", 128)], x=(n - 1, 0)))
        T.append(Case(s + "drle_longer_than_window", "xyz_u16", n, "front", [3], [("noise", 7)], x=(n - 1, 0),
                      note="one run per value: the section begins in front of the window"))
        # a false candidate 03 r 00 00 00 (x + 1 step, y + 5 steps, z NaN, then x NaN, y NaN at the next point), r = 11, with
        # 2 r = 22 ends behind it: 1 (z) + 3 * 5 (points) + 6 (the one-run Rle section)
        p = n - 7
        T.append(Case(s + "drle_false_alone", "xyz_u16", n, "drle_end", [2], rle, right=False, x=(n // 2, 0),
                      nan={"z": [p], "x": [p + 1], "y": [p + 1]}, plus={"x": [(p, 1)], "y": [(p, 5)]}, cols=0, sec_done=1))
        # ... and next to a real DeltaRle section of 2 runs (03 02 00 00 00 + 4 tokens: 9 ends): 22 = 1 + 3 * 4 + 9
        p = n - 6
        T.append(Case(s + "drle_false_next_to_real", "xyz_u16", n, "front", [3], [("runs", n, [7])], x=(n // 2, 0),
                      nan={"z": [p], "x": [p + 1], "y": [p + 1]}, plus={"x": [(p, 1)], "y": [(p, 5)]},
                      note="two candidates: no guess"))
        # ---- the count from the front
        T.append(Case(s + "front_two_fields", "xyz_u16_u16", n, "front", [0, 3], [_dv(n, b2=n // 3), ("ring", 64)], x=(n - 1, 0)))
        T.append(Case(s + "front_4ops_rle", "xyzi_u16", n, "front", [2], [("runs", 700, [0x9191, 0x9292])], x=(n // 3, 0)))
        # the last regular token ends on the last byte of a wave's part / on the first byte of the next part (PART: bytes of a
        # wave, stage1_decode_fast.h: `part`); the payloads' sizes are no multiples of 16
        for what, pn, b2, two, k in FRONT_PART[nw]:
            T.append(Case(s + "front_" + what, "xyz_u16_u16", pn, "front", [0, 0], [_dv(pn), _dv(pn, b2=b2)], x=(two, 0),
                          size=5 * pn + 2 + b2 + two, section=2 * pn + 2 + b2, part_k=k))
        # ---- DeltaVarint guess, wrong (b): a Palette section of 1793 entries whose every byte is part of a non-zero token of 1
        # or 3 bytes (big_palette_section below) -- E = 3 + 1196 + 11 n / 24 ends -- behind a regular stream whose token number
        # 2 n - 1 + E is the LAST marker: exactly n tokens of 1..5 bytes end behind it and k_section_dv_w completes a column
        e = 3 + 1196 + 11 * n // 24
        T.append(Case(s + "dv_wrong_garbage_column", "xyz_u16", n, "dv_end", [2], rle, right=False, nan=_marker(2 * n - 1 + e),
                      x=(0, n - 1), cols=1, sec_done=1, dv_chunks=1, split=(0, 1), assemble=True))
    return T


def big_palette_section(n, seed=1):
    """A Palette section (mode 1) of 1793 = 0x0701 entries for n values, written byte by byte: no byte is 0, the table's bytes
    end a token at every third byte from its first, the index bytes at every third byte from their third, and every 11-bit index
    is below 1793. The reference's encoder lists a palette in order of first occurrence and would not write it; its decoder
    (decodeV5AdaptiveIntSection) takes any table."""
    assert n % 24 == 0
    u = 0x0701
    rs = np.random.RandomState(seed)
    tab = 1 + rs.randint(0, 0x7F, 2 * u)
    tab[np.arange(2 * u) % 3 != 0] |= 0x80
    nb = 11 * n // 8
    idx = np.zeros(nb, dtype=np.int64)
    acc, held = 0, 0                       # bits of the indexes not yet complete
    for i in range(nb):
        for _try in range(64):
            b = (1 + int(rs.randint(0, 0x7F))) | (0x80 if i % 3 != 2 else 0)
            a, h, ok = acc | (b << held), held + 8, True
            while h >= 11:
                ok = ok and (a & 0x7FF) < u
                a >>= 11
                h -= 11
            if ok:
                break
        assert ok
        idx[i], acc, held = b, a, h
    return np.concatenate([[1, u & 0xFF, u >> 8], tab, idx]).astype(np.uint8)


# (name, points, 2-byte tokens of the second field, 2-byte x tokens, k): two DeltaVarint fields, the regular stream's last byte is
# the last byte of wave k - 1's part of the count from the front / the first byte of wave k's; found once with
# locate_model.front_part_bytes
FRONT_PART = {4: (("part_last_byte", 5400, 5400, 24, 2), ("part_first_byte", 5400, 5400, 25, 2)),
              16: (("part_last_byte", 21600, 0, 7360, 10), ("part_first_byte", 21600, 0, 7361, 10))}
CASES = _table()
BY_NAME = {c.name: c for c in CASES}
