"""Hand-built payloads for the device LZ4 encoder (cloudini_amd/csrc/lz4_kernels.hip), one per threshold and side of it.

The tool: INT8 / UINT8 fields are raw copies (FieldEncoderCopy), so for a schema of K UINT8 fields with
point_step K the stage-1 payload of a chunk IS that chunk's point bytes. RAW1 puts N payload bytes in a cloud of N points
(chunks of 32 KiB), RAW4 gives 128 KiB chunks, RAW32 1 MiB chunks (128 sub-ranges, 256 under the FAST parameters).

A case is a cloud (family k: a list of clouds) plus the condition the model's trace (Oracle.lz4_trace) must meet, so that a
case provably reaches the branch it was built for. The trace never supplies expected bytes: those are Oracle.lz4_model's.
Nothing here touches a GPU; tests/test_lz4_payload_grid.py holds the conditions on the CPU, tests/test_gpu_lz4_encode_grid.py
runs the cases on the device.

Building blocks: a filler without a match (FILL, asserted by a CPU test for every sub-range at both parameter sets) and
planted copies: the bytes at q - 70 copied to q, the source in the steps before the match's, the bytes in front of and behind
every copy made to differ, so that positions and lengths are exact. A source is overwritten in the hash table when a position
between it and the match's step hashes to the same slot; plant() sees that (the hash is restated here) and the case is then
built on the next stretch of the filler.

Families (the issue's letters):
  a  size edges, RAW1: n = 1..24, 63..65, around SUB and 2 * SUB, 32767..32769, as zeros, period 7 and filler
  b  one match per case, RAW4: 24 lengths x 5 lanes, offsets on both sides of 256, matches cut by a sub-range end and by n - 5
  c  start limits: a copy at last_start (found) and one behind it (not found), last and inner sub-range
  d  a step of 16 matches (lane offsets 0 and 1) and one of 15 (lane offset 4)
  e  a step that runs past its end (cur > 64), a second match at cur and at cur + 1
  f  a full list: with the last step, halfway, one step short of full, capacity - 16 and - 15 with a copy behind, full next to empty
  g  literal runs of 0..271 bytes in front of a non-first sequence at every source x destination alignment mod 4
  h  first sequences across sub-range edges: skip0 == 0, a first match at s + 64, literals that begin 1, 2 and 65 sub-ranges earlier
  i  the span threshold of k_lz4_emit_lds: spans of SUB - 1 + x around kImg = SUB + 320, matches of 4, 20 and 274 bytes
  j  chunks of 1 MiB: matches in chosen sub-ranges only, in all, in none; lz_emit_direct with a full list and with g's runs
  k  1100 clouds of 13..40 bytes (the second round of k_lz4_plan and k_lz4_offsets)
"""
from __future__ import annotations

import numpy as np

import cases
from cloudini_amd.schema import FieldType

PARAMS = {1: (8192, 11, 1024), 2: (4096, 10, 512)}   # CLDN_HIP_STAGE2_LZ4, ..._FAST: sub-range bytes, hash bits, list capacity
K_IMG_EXTRA = 320                                     # kImg = SUB + 320 (k_lz4_emit_lds)
CHUNK_POINTS = 32768
STEPS = {"RAW1": 1, "RAW4": 4, "RAW32": 32}

FILL_SEED = 5
FILL_STRETCH = 8192
FILL_BYTES = (1 << 20) + 16 * FILL_STRETCH
_fill = None


def schema(name: str, n_points: int = 0):
    k = STEPS[name]
    return cases.make_info([(f"b{i}", i, FieldType.UINT8, None) for i in range(k)], k, n_points)


def fill_bytes() -> np.ndarray:
    global _fill
    if _fill is None:
        _fill = np.random.RandomState(FILL_SEED).randint(0, 256, FILL_BYTES).astype(np.uint8)
    return _fill


def filler(n: int, o: int = 0) -> np.ndarray:
    """n bytes of the filler from a sub-range aligned position: every sub-range of the result is the head of one of FILL's."""
    assert o % FILL_STRETCH == 0 and o + n <= FILL_BYTES
    return fill_bytes()[o:o + n].copy()


def chunk_payloads(schema_name: str, cloud: np.ndarray):
    cb = CHUNK_POINTS * STEPS[schema_name]
    return [cloud[o:o + cb] for o in range(0, cloud.size, cb)]


def ext_bytes(x: int) -> int:
    return (x - 15) // 255 + 1 if x >= 15 else 0


class Collision(Exception):
    pass


class Buf:
    """Filler with planted copies."""

    def __init__(self, n: int, P, o: int = 0):
        self.b = filler(n, o)
        self.sub, self.bits, self.mm = P

    def _hashes(self, lo: int, hi: int) -> np.ndarray:   # of positions lo .. hi - 1
        w = self.b[lo:hi + 3].astype(np.uint64)
        v = w[:-3] | (w[1:-2] << np.uint64(8)) | (w[2:-1] << np.uint64(16)) | (w[3:] << np.uint64(24))
        return ((v * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - self.bits)

    def plant(self, q: int, length: int, dist: int = 70, step=None, before: bool = True, behind: bool = True, check: bool = True):
        """Copy `length` bytes from q - dist to q (as an LZ4 decoder would: a length beyond dist repeats). `step` = the first
        position of the parser's step that holds q (default: steps of 64 from the sub-range start)."""
        b, src = self.b, q - dist
        s0 = (q // self.sub) * self.sub
        if step is None:
            step = s0 + ((q - s0) // 64) * 64
        assert s0 <= src < step, "the source is entered into the table in a step before the match's"
        length = min(length, b.size - q)                 # (a copy that would leave the payload ends with it)
        if before and src > s0 and b[q - 1] == b[src - 1]:
            b[q - 1] ^= 0xAA
        for k in range(length):
            b[q + k] = b[src + k]
        if behind and q + length < b.size and b[q + length] == b[src + length]:
            b[q + length] ^= 0x55
        if check and step > src + 1:
            h = self._hashes(src + 1, step)
            mine = int(self._hashes(q, q + 1)[0])
            for p in (np.nonzero(h == mine)[0] + src + 1):
                if b[p:p + 4].tobytes() != b[q:q + 4].tobytes():
                    raise Collision(f"position {p} takes the table slot of {src}")
        return self


class Case:
    def __init__(self, family, name, schema_name, clouds, cond):
        self.family, self.name, self.schema, self.clouds, self.cond = family, name, schema_name, clouds, cond
        step = STEPS[schema_name]
        for c in clouds:
            assert c.dtype == np.uint8 and c.size % step == 0, (family, name, c.size)

    @property
    def id(self):
        return f"{self.family}:{self.name}"


def _retry(fn):
    for t in range(16):
        try:
            return fn(t * FILL_STRETCH)
        except Collision:
            continue
    raise AssertionError("no stretch of the filler without a collision")


def _up(n: int, k: int) -> int:
    return (n + k - 1) // k * k


def pl(t):
    """(pos, len) of every match of a chunk's trace"""
    return [(int(r[0]), int(r[1])) for r in t.matches]


def plo(t):
    return [(int(r[0]), int(r[1]), int(r[2])) for r in t.matches]


# ---- a. size edges -------------------------------------------------------------------------------------------------------------
def _family_a(P):
    sub = P[0]
    sizes = list(range(1, 25)) + [63, 64, 65, sub - 1, sub] + [sub + k for k in range(1, 14)] + [2 * sub - 1, 2 * sub, 32767, 32768, 32769]
    out = []
    for n in sorted(set(sizes)):
        forms = {"zeros": np.zeros(n, np.uint8), "period7": np.resize(np.arange(7, dtype=np.uint8), n), "filler": filler(n)}
        for form, data in forms.items():
            def cond(T, n=n, form=form):
                assert len(T) == (n + CHUNK_POINTS - 1) // CHUNK_POINTS
                for t in T:
                    m = plo(t)
                    if t.n < 13:
                        assert not m
                    for pos, ln, _ in m:
                        assert pos <= t.n - 12 and pos + ln <= t.n - 5
                    if form == "filler":
                        assert not m
                        continue
                    for k, r in enumerate(t.subs):                     # zeros and period 7: one match to where matches may end
                        limit = min(int(r["e"]), t.n - 5) if t.n >= 13 else 0
                        if int(r["count"]):
                            assert int(r["last_end"]) == limit, (k, r)
                        if limit - int(r["s"]) >= 128 and t.n >= 13:
                            assert int(r["count"]) >= 1
            out.append(Case("a", f"{form}_{n}", "RAW1", [data], cond))
    return out


# ---- b. one match per case -------------------------------------------------------------------------------------------------------
MATCH_LENGTHS = [4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 19, 20, 79, 80, 81, 143, 144, 145, 273, 274, 529]   # and SUB - 200
LANES = [0, 1, 31, 62, 63]
CUT_LENGTHS = [4, 5, 8, 12, 15, 16, 17, 80, 81]
MATCH_OFFSETS = [64, 255, 256, 257, 511, 512, 1000]


def _family_b(P):
    sub = P[0]
    out = []
    for ln in MATCH_LENGTHS + [sub - 200]:
        for lane in LANES:
            q = 128 + lane
            n = _up(q + ln + 64, 4)
            data = _retry(lambda o: Buf(n, P, o).plant(q, ln).b)
            out.append(Case("b", f"len{ln}_lane{lane}", "RAW4", [data],
                            lambda T, q=q, ln=ln: _assert_eq(plo(T[0]), [(q, ln, 70)])))
    for dist in MATCH_OFFSETS:                              # both bytes of the offset field
        q = 128 + _up(dist, 64) + 5
        data = _retry(lambda o: Buf(_up(q + 8 + 64, 4), P, o).plant(q, 8, dist=dist).b)
        out.append(Case("b", f"offset{dist}", "RAW4", [data], lambda T, q=q, dist=dist: _assert_eq(plo(T[0]), [(q, 8, dist)])))
    for c in CUT_LENGTHS:
        # cut by the end of an inner sub-range: the copy goes on behind e, the match does not
        n = sub + 256
        q = sub - c
        data = _retry(lambda o: Buf(n, P, o).plant(q, c + 20).b)
        out.append(Case("b", f"cut{c}_at_sub_end", "RAW4", [data], lambda T, q=q, c=c: _assert_eq(plo(T[0]), [(q, c, 70)])))
        # cut by n - 5: the copy goes on to n. A match of 4 or 5 bytes that ends at n - 5 would start behind n - 12: not found
        n = 512
        q = n - 5 - c
        data = _retry(lambda o: Buf(n, P, o).plant(q, n - q).b)
        want = [(q, c, 70)] if q <= n - 12 else []
        out.append(Case("b", f"cut{c}_at_n_minus_5", "RAW4", [data], lambda T, want=want: _assert_eq(plo(T[0]), want)))
    return out


def _assert_eq(got, want):
    assert got == want, (got, want)


# ---- c. start limits -------------------------------------------------------------------------------------------------------------
def _family_c(P):
    sub = P[0]
    out = []
    for where, n, last_start, limit in (("last", 512, 512 - 12, 512 - 5), ("inner", sub + 256, sub - 4, sub)):
        for d in (0, 1):
            q = last_start + d
            data = _retry(lambda o: Buf(n, P, o).plant(q, 12).b)
            want = [] if d else [(q, limit - q, 70)]
            out.append(Case("c", f"{where}_last_start_plus_{d}", "RAW4", [data], lambda T, want=want: _assert_eq(plo(T[0]), want)))
    return out


# ---- d. a step of 16 matches -------------------------------------------------------------------------------------------------------
def _family_d(P):
    out = []
    for off, in_step in ((0, 16), (1, 16), (4, 15)):
        # 16 words of the filler with a separator behind each at 128.., back to back at 256 + off
        def build(o):
            bf = Buf(512, P, o)
            b = bf.b
            a, q = 128, 256 + off
            for k in range(16):
                w = a + 5 * k
                nxt = b[w + 5] if k < 15 else b[q + 64]
                if b[w + 4] == nxt:
                    b[w + 4] ^= 0x55                       # the separator differs from what follows the word's copy
            for k in range(16):
                bf.plant(q + 4 * k, 4, dist=q + 4 * k - (a + 5 * k), step=256, before=False, behind=False)
            return b
        data = _retry(build)

        def cond(T, off=off, in_step=in_step):
            t = T[0]
            assert pl(t) == [(256 + off + 4 * k, 4) for k in range(16)]
            steps = {int(r[0]): (int(r[1]), int(r[2])) for r in t.steps}
            assert steps[256] == (in_step, 60 + off if in_step == 15 else 64 + off)
            if in_step == 15:
                assert steps[320] == (1, 4)
        out.append(Case("d", f"lane_offset_{off}", "RAW4", [data], cond))
    return out


# ---- e. a step that runs past its end ------------------------------------------------------------------------------------------
def _family_e(P):
    out = []
    for ln in (5, 68, 200):
        for behind in (None, 0, 1):
            q = 128 + 60
            q2 = None if behind is None else q + ln + behind

            def build(o):
                bf = Buf(1024, P, o).plant(q, ln)
                if q2 is not None:
                    bf.plant(q2, 6, dist=90, step=q + ln, before=bool(behind), check=ln < 70)
                return bf.b
            data = _retry(build)

            def cond(T, ln=ln, q=q, q2=q2):
                t = T[0]
                assert pl(t) == [(q, ln)] + ([(q2, 6)] if q2 is not None else [])
                steps = [(int(r[0]), int(r[1]), int(r[2])) for r in t.steps]
                k = [r[0] for r in steps].index(128)
                assert steps[k] == (128, 1, 60 + ln) and steps[k][2] > 64
                # the following step starts where the match ended: unaligned for 5 and 200 bytes, two steps on for 68
                assert steps[k + 1][0] == q + ln and (q + ln) % 64 == {5: 1, 68: 0, 200: 4}[ln]
                if q2 is not None:
                    assert steps[k + 1][1] == 1                                   # and finds the second match at lane 0 / 1
            out.append(Case("e", f"len{ln}_second_{'none' if behind is None else behind}", "RAW4", [data], cond))
    return out


# ---- f. a full list --------------------------------------------------------------------------------------------------------------
def _repeats(bf, s, first, period, count, limit):
    """a 4-byte repeat (from 70 back) every `period` bytes from s + first on: `count` of them at most, none beyond `limit`"""
    q, k = s + first, 0
    while k < count and q + 5 <= limit:
        bf.plant(q, 4, before=False, check=False)
        q += period
        k += 1
    return k


# A repeat every 6 bytes is not found every time (a later position may take its source's table slot), so two numbers are
# read off the model's trace, per parameter set, and held by the cases' conditions: the payload size at which the step that
# fills the list is the chunk's last one, and the number of repeats that leaves the list 16 entries short of its capacity.
FILLS_WITH_LAST_STEP = {8192: 6804, 4096: 3440}
ONE_STEP_SHORT = {8192: 1118, 4096: 551}
# ... and the numbers of repeats, all in front of SUB - 600, of which the model finds capacity - 16 and capacity - 15: a step
# is parsed while count + 16 <= capacity, so a copy at SUB - 400 is found behind the first and left as literals behind the second
CAP_MINUS_16 = {8192: 1118, 4096: 555}
CAP_MINUS_15 = {8192: 1119, 4096: 556}


def _family_f(P):
    sub, _bits, mm = P
    out = []

    def one(name, n, plan, cond, schema_name="RAW4"):
        def build(o):
            bf = Buf(n, P, o)
            plan(bf)
            return bf.b
        out.append(Case("f", name, schema_name, [build(0)], cond))

    # the list fills with the sub-range's last step: nothing is left to parse
    def cond_last(T):
        r = T[0].subs[0]
        assert int(r["count"]) + 16 > mm and not int(r["full"]), r
    n_last = FILLS_WITH_LAST_STEP[sub]
    one("fills_with_the_last_step", n_last, lambda bf: _repeats(bf, 0, 72, 6, 1 << 20, n_last), cond_last)

    # the list fills halfway (a repeat every 5 bytes): the repeats behind the cap leave as literals
    def cond_half(T):
        r = T[0].subs[0]
        assert int(r["full"]) and int(r["count"]) + 16 > mm and int(r["last_end"]) < sub - sub // 4, r
        assert int(T[0].subs[1]["count"]) == 0
    one("fills_halfway", sub + 256, lambda bf: _repeats(bf, 0, 72, 5, 1 << 20, sub), cond_half)

    # one step short of full: mm - 16 matches, the parser goes on to the end and finds nothing more
    def cond_short(T):
        r = T[0].subs[0]
        assert mm - 24 < int(r["count"]) <= mm - 16 and not int(r["full"]), r
    one("one_step_short", sub + 256, lambda bf: _repeats(bf, 0, 72, 6, ONE_STEP_SHORT[sub], sub), cond_short)

    # the list's last admitted step: count + 16 == capacity is parsed, count + 16 == capacity + 1 is not
    def plan_cap(table):
        def plan(bf):
            assert _repeats(bf, 0, 72, 6, table[sub], sub - 600) == table[sub]
            bf.plant(sub - 400, 9)
        return plan

    def cond_cap16(T):
        r = T[0].subs[0]
        assert int(r["count"]) == mm - 15 and pl(T[0])[-1] == (sub - 400, 9) and pl(T[0])[-2][0] < sub - 600, r
    one("capacity_minus_16_then_a_match", sub + 256, plan_cap(CAP_MINUS_16), cond_cap16)

    def cond_cap15(T):
        r = T[0].subs[0]
        assert int(r["count"]) == mm - 15 and int(r["full"]) and pl(T[0])[-1][0] < sub - 600, r
    one("capacity_minus_15_then_a_copy", sub + 256, plan_cap(CAP_MINUS_15), cond_cap15)

    # a full sub-range between two without a match
    def cond_nb(T):
        s = T[0].subs
        assert [int(x) for x in s["count"][[0, 2]]] == [0, 0] and int(s["full"][1]) and int(s["count"][1]) + 16 > mm
    one("full_between_empty", 3 * sub, lambda bf: _repeats(bf, sub, 72, 5, 1 << 20, 2 * sub), cond_nb)
    return out


# ---- g. literal runs in front of a non-first sequence --------------------------------------------------------------------------
LITERAL_RUNS = [0, 1, 2, 3, 14, 15, 16, 127, 128, 129, 269, 270, 271]


def _family_g(P):
    """[p filler][match of 4 + d bytes][the run][match of 4 bytes][filler]: the run starts at p + 4 + d in the payload and
    behind 1 + ext + p + 2 block bytes, so p = 128..131 with d = 0..3 gives it every source x destination alignment mod 4."""
    out = []
    for run in LITERAL_RUNS:
        for p in range(128, 132):
            for d in range(4):
                q1 = p + 4 + d + run
                step1 = (q1 // 64) * 64                   # (the first match ends at 138 at the latest: the steps stay aligned)

                def build(o):
                    bf = Buf(q1 + 4 + 32, P, o).plant(p, 4 + d)
                    for dist in (90, 110, 125):
                        src = q1 - dist
                        if src >= 0 and src + 5 < step1 and (src + 6 < p - 71 or src > p - 66 + d + 2):
                            return bf.plant(q1, 4, dist=dist, step=step1, before=run > 0).b
                    raise AssertionError("no source for the second match")
                data = _retry(build)
                out.append(Case("g", f"run{run}_p{p}_d{d}", "RAW1", [data],
                                lambda T, p=p, d=d, q1=q1: _assert_eq(pl(T[0]), [(p, 4 + d), (q1, 4)])))
    return out


# ---- h. first sequences across sub-range edges -----------------------------------------------------------------------------------
def _family_h(P):
    sub = P[0]
    out = []

    # the previous match ends exactly at e: the first sequence of the next sub-range has no literal in front of s
    def build(o):
        return Buf(2 * sub, P, o).plant(sub - 20, 40).plant(sub + 130, 6).b

    def cond(T):
        t = T[0]
        assert pl(t) == [(sub - 20, 20), (sub + 130, 6)]
        assert int(t.subs[1]["anchor_in"]) == sub and int(t.subs[1]["skip0"]) == 0 and int(t.subs[1]["lit0"]) == 130
    out.append(Case("h", "previous_match_ends_at_e", "RAW4", [_retry(build)], cond))

    # a first match at s + 64, the earliest position a sub-range can find one at (its table is empty during the first step,
    # so a match AT s, skip0 == lit0, cannot occur): all literals but 64 lie in the sub-range before
    def build64(o):
        bf = Buf(2 * sub, P, o).plant(200, 8)
        bf.b[sub + 64:sub + 72] = bf.b[sub:sub + 8]
        if bf.b[sub + 72] == bf.b[sub + 8]:
            bf.b[sub + 72] ^= 0x55
        return bf.b

    def cond64(T):
        t = T[0]
        assert pl(t) == [(200, 8), (sub + 64, 8)]
        r = t.subs[1]
        assert int(r["skip0"]) == sub - 208 and int(r["lit0"]) == int(r["skip0"]) + 64
    out.append(Case("h", "first_match_at_s_plus_64", "RAW4", [build64(0)], cond64))

    # literals that begin 1, 2 and 65 sub-ranges earlier
    for back in (1, 2, 65):
        name = "RAW32" if back == 65 else "RAW4"
        k1 = back + 1
        n = (k1 + 1) * sub

        def build(o, k1=k1, n=n):
            return Buf(n, P, o).plant(300, 9).plant(k1 * sub + 500, 9).b

        def cond(T, k1=k1, back=back):
            t = T[0]
            assert pl(t) == [(300, 9), (k1 * sub + 500, 9)]
            r = t.subs[k1]
            assert int(r["anchor_in"]) == 309 and int(r["skip0"]) == k1 * sub - 309 and int(r["lit0"]) == int(r["skip0"]) + 500
            assert int(t.subs[0]["next_pos"]) == k1 * sub + 500
            assert all(int(x) == 0 for x in t.subs["count"][1:k1])
        out.append(Case("h", f"literals_begin_{back}_sub_ranges_earlier", name, [_retry(build)], cond))
    return out


# ---- i. the span threshold -----------------------------------------------------------------------------------------------------
SPAN_X = [300, 305, 306, 307, 308] + list(range(313, 324)) + [325, 330, 400]


def _family_i(P):
    """One match at 1000, filler to the end: sub-range 0's span is its sequence, the header of the block's last sequence and
    the bytes behind the match: SUB + 3 + ext(len - 4) + X - len with X = the extension bytes of that header. For a 4-byte
    match that is SUB - 1 + X; the longer matches get the X that gives the same span. The payload size is the smallest
    multiple of the schema's point step with X extension bytes (a range of 255 sizes has them)."""
    sub = P[0]
    k_img = sub + K_IMG_EXTRA
    out = []
    for ln in (4, 20, 274):
        for x in SPAN_X:
            big_x = x + ln - 4 - ext_bytes(ln - 4)
            name = "RAW4" if 1000 + ln + 15 + 255 * big_x <= CHUNK_POINTS * 4 else "RAW32"
            n = _up(1000 + ln + 15 + 255 * (big_x - 1), STEPS[name])
            assert ext_bytes(n - 1000 - ln) == big_x and n <= CHUNK_POINTS * STEPS[name]
            data = _retry(lambda o: Buf(n, P, o).plant(1000, ln).b)

            def cond(T, ln=ln, x=x):
                t = T[0]
                assert len(T) == 1 and plo(t) == [(1000, ln, 70)]
                span = int(t.subs[0]["span"])
                assert span == sub - 1 + x
                if x <= 306:
                    assert span + 15 <= k_img
                elif x >= 322:
                    assert span > k_img
                else:
                    assert span <= k_img < span + 15                          # the address decides
                assert all(int(s) <= sub for s in t.subs["span"][1:])
            out.append(Case("i", f"len{ln}_x{x}", name, [data], cond))
    return out


# ---- j. chunks of 1 MiB ----------------------------------------------------------------------------------------------------------
def _family_j(P):
    sub = P[0]
    n = 1 << 20
    n_subs = n // sub
    last = n_subs - 1
    out = []
    for name, where in (("first_and_last", [0, last]), ("sub_70", [70]), ("subs_63_64", [63, 64]), ("all", list(range(n_subs))), ("none", [])):
        # (with up to 256 copies one stretch of the filler without any collision does not exist: a copy whose source is
        # overwritten moves on by a step inside its sub-range instead)
        bf, at = Buf(n, P), []
        for k in where:
            for q in range(k * sub + 138, k * sub + 138 + 64 * 16, 64):
                keep = bf.b[q - 1:q + 9].copy()
                try:
                    bf.plant(q, 8)
                    at.append(q)
                    break
                except Collision:
                    bf.b[q - 1:q + 9] = keep
        assert len(at) == len(where)

        def cond(T, at=at):
            t = T[0]
            assert len(T) == 1 and len(t.subs) == n_subs > 64
            assert pl(t) == [(q, 8) for q in at]
            for k in (0, 62, 63, 64, last - 1):                                # next_pos: the first match behind, tiles of 64 away
                behind = [q for q in at if q >= (k + 1) * sub]
                assert int(t.subs[k]["next_pos"]) == (behind[0] if behind else n)
            if not at:
                assert t.size == 1 + ext_bytes(n) + n and ext_bytes(n) > 4100
        out.append(Case("j", name, "RAW32", [bf.b], cond))

    # lz_emit_direct with work of every kind: sub-range 0 holds sequences, the rest of the MiB is one literal run, so the
    # header behind sub-range 0 has about 4000 extension bytes and its span does not fit the image
    def direct(T, m_min):
        t = T[0]
        r = t.subs[0]
        assert int(r["count"]) >= m_min and int(r["gap"]) > 4000 and int(r["span"]) > sub + K_IMG_EXTRA + 1000
        assert all(int(x) == 0 for x in t.subs["count"][1:])

    # ... a full list (more than 64 sequences: tiles of 64 in the direct path too), matchable data behind the cap
    bf = Buf(n, P)
    _repeats(bf, 0, 72, 5, 1 << 20, sub)
    out.append(Case("j", "direct_full_list", "RAW32", [bf.b], lambda T: (direct(T, P[2] - 15), _assert_eq(int(T[0].subs[0]["full"]), 1))))

    # ... the literal runs of family g in one chain, matches of 4..7 bytes between them
    def chain(o):
        bf = Buf(n, P, o)
        b, q, planned = bf.b, 130, []
        i, last_end = 128, 0                                    # the parser's step that holds the latest match, where that ends
        for k, run in enumerate([5] + LITERAL_RUNS + LITERAL_RUNS[::-1]):
            q += run
            ln = 4 + k % 4
            while q >= i + 64:                                  # (a step moves on by 64, or to the end of its last match)
                i, last_end = i + max(64, last_end - i), 0
            for dist in range(70, 400, 9):
                src = q - dist
                if not (0 <= src and src + ln + 1 < i and all(src + ln + 2 < s2 or src > s2 + l2 + 2 for _q, l2, s2 in planned)):
                    continue
                keep = b[q:q + ln].copy()
                try:
                    bf.plant(q, ln, dist=dist, step=i, before=False, behind=False)
                except Collision:
                    b[q:q + ln] = keep
                    continue
                planned.append((q, ln, src))
                break
            else:
                raise Collision("no source")
            q += ln
            last_end = q
        for q, ln, src in planned:                              # lengths and positions are exact
            if b[q + ln] == b[src + ln] or b[q - 1] == b[src - 1]:
                raise Collision("a copy would run on")
        return b, [(q, ln) for q, ln, _ in planned]
    data, planned = _retry(chain)
    out.append(Case("j", "direct_literal_runs", "RAW32", [data],
                    lambda T: (direct(T, len(planned)), _assert_eq(pl(T[0]), planned))))
    return out


# ---- k. many chunks ----------------------------------------------------------------------------------------------------------------
def _family_k(P):
    clouds = []
    for k in range(1100):
        n = 13 + k % 28
        kind = k % 3
        clouds.append(np.zeros(n, np.uint8) if kind == 0 else np.resize(np.arange(7, dtype=np.uint8), n) if kind == 1 else filler(n))

    def cond(T):
        assert len(T) == 1100 > 1024                                            # one chunk each: a second round of 1024
        assert all(13 <= t.n <= 40 and len(t.subs) == 1 for t in T)
    return [Case("k", "1100_clouds", "RAW1", clouds, cond)]


FAMILIES = {"a": _family_a, "b": _family_b, "c": _family_c, "d": _family_d, "e": _family_e, "f": _family_f, "g": _family_g,
            "h": _family_h, "i": _family_i, "j": _family_j, "k": _family_k}
_grids = {}


def grid(stage2: int):
    """every case for one parameter set (built once)"""
    if stage2 not in _grids:
        _grids[stage2] = [c for f in sorted(FAMILIES) for c in FAMILIES[f](PARAMS[stage2])]
    return _grids[stage2]


def batches(stage2: int):
    """(family, schema) -> the cases that go into one encode call, in file order"""
    out = {}
    for c in grid(stage2):
        out.setdefault((c.family, c.schema), []).append(c)
    return out


BATCH_KEYS = [("a", "RAW1"), ("b", "RAW4"), ("c", "RAW4"), ("d", "RAW4"), ("e", "RAW4"), ("f", "RAW4"), ("g", "RAW1"), ("h", "RAW4"),
              ("h", "RAW32"), ("i", "RAW4"), ("i", "RAW32"), ("j", "RAW32"), ("k", "RAW1")]
