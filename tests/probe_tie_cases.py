"""Integer columns whose adaptive-mode section sizes lie within one byte of each other, shared by tests/test_probe_tie_cases.py
(model against oracle and reference, coverage, sensitivity) and tests/test_gpu_probe_ties.py (the three probe kernels and the
mode sweep against the model). No GPU, no library code.

The probe commits argmin(DeltaVarint, Palette, Rle, DeltaRle) with strict '<' in that order over the first min(n, 4096) values;
the sizes never leave the kernel. A size term that is off by one shows only where two sizes lie within one byte of each other,
so every row here is built to such a place, and carries a predicate `cond` on mode_model.section_sizes(values[:4096], bpv) that
must hold before the row is used anywhere: a row can never pass for the wrong reason.

Rows are (name, family, ftype, values, cond); `values` has the numpy type of ftype. Construction is closed form: every family
of columns has a knob that moves size[a] - size[b] by a known whole number of bytes per step (and, where that number is not
one, a second knob that moves it by one), so the knobs that give a wanted difference follow from the sizes of one trial column
by division -- _settle() does that division and checks the result, it does not search. Nothing is random.

Families
  pair   every unordered pair of modes x (size[a] - size[b]) in {-1, 0, +1} x width in {2, 4, 8}, the two other modes at least
         2 bytes above the smaller of the pair; length classes mid (1025 < n < 4096, n % 16 != 0), full (n == 4096) and beyond
         (the full row's window with values behind it that make the pair's loser the best mode of the whole cloud by >= 64 bytes)
  term   triples (tie, minus, plus): the tie, and the two neighbours in which ONE size term of one mode is one byte smaller /
         larger and nothing else has changed (TERMS names the mode; the predicate asserts the other three sizes are the tie's)
  tiny   every column of length 1..4 over {0, 1, 63, 64, type max, all-ones}
  sums   two-chunk clouds (32768 + 300 values): a clear winner in each chunk, the sums over the chunks within one byte

UNREACHED at the end of the file lists the cells that are not here, and why."""
from __future__ import annotations

import itertools

import numpy as np

import cases
import mode_model as M

F = cases.F
DV, PAL, RLE, DRLE = range(4)
MODE_NAMES = ("dv", "pal", "rle", "drle")
PAIRS = list(itertools.combinations(range(4), 2))
DIFFS = (-1, 0, 1)
WIDTHS = (2, 4, 8)
TYPES_OF = {2: (F.UINT16, F.INT16), 4: (F.UINT32, F.INT32), 8: (F.UINT64, F.INT64)}
NP = {F.UINT16: np.uint16, F.INT16: np.int16, F.UINT32: np.uint32, F.INT32: np.int32, F.UINT64: np.uint64, F.INT64: np.int64}
SIGNED = {F.INT16, F.INT32, F.INT64}
WIDTH_OF = {t: w for w, ts in TYPES_OF.items() for t in ts}
PROBE, CHUNK = M.PROBE, M.CHUNK
MID_N = {2: 2003, 4: 3001, 8: 3517}     # > 1025, no multiple of 16: more than one wave of 256 and of 1024 values, a partial last thread
TAIL_MARGIN = 64
TERM_N = 4093                          # the term triples: mid class, room for a run that starts at 960


def typed(v, ftype):
    """Whole numbers (int64; for the 64-bit types the int64 the model sees) as the field's own type; they must fit it."""
    v = np.asarray(v, dtype=np.int64)
    if ftype == F.UINT64:
        return v.view(np.uint64)
    ii = np.iinfo(NP[ftype])
    assert v.size == 0 or (ii.min <= int(v.min()) and int(v.max()) <= ii.max), (ftype, int(v.min()), int(v.max()))
    return v.astype(NP[ftype])


def as_model(values):
    """ToInt64<T> of the reference: what mode_model.column() returns for the row's field."""
    values = np.asarray(values)
    return values.view(np.int64) if values.dtype == np.uint64 else values.astype(np.int64)


def window_sizes(values):
    return M.section_sizes(as_model(values)[:PROBE], np.asarray(values).dtype.itemsize)


def whole_sizes(values):
    """The sums over the chunks: what the sweep reports as bytes[0..3]."""
    v, w = as_model(values), np.asarray(values).dtype.itemsize
    return [int(x) for x in np.sum([M.section_sizes(v[c:c + CHUNK], w) for c in range(0, v.size, CHUNK)], axis=0)]


# ---- column families: whole numbers >= 0 from two knobs --------------------------------------------------------------------

# the smallest |delta| whose token has v bytes is 2^(7v - 8) (v >= 2); per width: a delta of w - 1 bytes, and one of w bytes
D_SHORT = {2: 20, 4: 9000, 8: (1 << 41) + 12345}
D_LONG = {2: 64, 4: 1 << 20, 8: 1 << 48}
TOP = {2: 30000, 4: 1 << 30, 8: 1 << 60}   # run heads bounce between 0 and TOP: half the signed type's range


def _split(total, parts, lo, hi):
    """`parts` lengths in [lo, hi] that sum to `total`, as even as they can be."""
    assert parts > 0, (total, parts)
    base, extra = divmod(total, parts)
    assert lo <= base and base + (1 if extra else 0) <= hi, (total, parts, lo, hi)
    return [base + 1] * extra + [base] * (parts - extra)


def _bounce(deltas, top):
    """Run heads: 0, then each delta added, or subtracted where adding would leave [0, top]."""
    out, cur, sign = [0], 0, 1
    for d in deltas:
        if not 0 <= cur + sign * d <= top:
            sign = -sign
        cur += sign * d
        out.append(cur)
    return np.array(out, dtype=np.int64)


def _dv_pal(n, w, z, _u, count=200):
    """`count` values, a lower half 0, 1, .. and an upper half 1000, 1001, ..; no value and no delta twice in a row. z values zig-zag
    between the halves (every delta has two bytes), the rest walks the lower half by +-1, +-2 (one byte):
    DeltaVarint = n + z + c, Palette = 3 + count w + ceil(bits n / 8)."""
    half = count // 2
    assert 2 * (count - half) <= z - 1 <= n - 4 and 100 <= half <= 128, (n, z, count)
    j = np.arange(z - (z & 1))                                  # an even number: from the lower half to the upper
    out = list(np.where(j % 2 == 0, (j // 2) % half, 1000 + (j // 2) % (count - half))) + [10] + [74] * (z & 1)   # back, and once more 64
    return np.array(out + _walk(out[-1], n - len(out), half - 1), dtype=np.int64)


def _walk(cur, count, top):
    """`count` values behind `cur`: steps of 1, 2, 1, 2, .. up to `top`, down to 0 and up again."""
    out, up = [], True
    for t in range(count):
        d = 1 + (t & 1)
        if up and cur + d > top:
            up = False
        elif not up and cur - d < 0:
            up = True
        cur += d if up else -d
        out.append(cur)
    return out


def _dv_rle(n, w, r, u):
    """r runs of 2..127 equal values whose heads are w - 1 token bytes apart (u of them: w bytes).
    DeltaVarint = 1 + n + r (w - 2) + u, Rle = 5 + r (w + 1), DeltaRle = 5 + r (w + 2) + u, the heads distinct for a long while."""
    assert 0 <= u < r
    deltas = [D_SHORT[w]] * (r - 1)
    deltas[:u] = [D_LONG[w]] * u
    return np.repeat(_bounce(deltas, TOP[w]), _split(n, r, 2, 127))


_PAT = (5, -3, 7, -4, 6, -2)


def _dv_drle(n, w, k, _u):
    """Runs of two equal deltas, neighbours different, no delta zero: a run of one-byte deltas costs both codings 2 bytes. k > 0: each
    of the first k runs (two-byte deltas) costs DeltaVarint 4 and DeltaRle 3. k < 0: -k single deltas in front (1 and 2 bytes)."""
    assert -1024 <= k <= 64
    if k >= 0:
        d = np.repeat([64 + i for i in range(k)] + [_PAT[i % 6] for i in range((n + 1) // 2 - k)], 2)
    else:
        # (where that leaves an odd number of values, the last run is one more single: a run of two-byte deltas makes up for it)
        big = [64, 64] * ((n + k) & 1)
        d = np.concatenate([[8 + i % 3 for i in range(-k)], big, np.repeat([_PAT[i % 6] for i in range((n + k + 1) // 2)], 2)])
    return np.cumsum(d[:n]).astype(np.int64)


PAL_STEP = {2: 1, 4: 1 << 13, 8: 1 << 41}  # sixteen palette values this far apart: a head's delta has w - 1 bytes or more


def _pal_rle_lens(lens, w):
    return np.repeat((np.arange(len(lens)) % 16) * PAL_STEP[w], lens)


def _pal_rle(n, w, r, u):
    """16 values in r runs, u of them of 128 values, the others of 2..127: Palette = 3 + 16 w + ceil(n / 2), Rle = 5 + r (w + 1) + u."""
    assert 0 <= u <= r - 16
    return _pal_rle_lens([128] * u + _split(n - 128 * u, r - u, 2, 127), w)


def _pal_drle(n, w, k, u):
    """k ramps 0, 5, 10, ... of 2..16 values, each a run of +5 and one jump back; the u ramps of 14 values or more jump back by
    65 or more (two bytes): Palette = 3 + 16 w + ceil(n / 2), DeltaRle = 5 + 4 k + u + c, DeltaVarint = 1 + n + u + c."""
    assert 1 <= u < k
    lens = [16] + [14] * (u - 1) + _split(n - 16 - 14 * (u - 1), k - u, 2, 13)
    return np.concatenate([np.arange(l) * 5 for l in lens]).astype(np.int64)


RAMP = {2: 100, 4: 60, 8: 40}


def _rle_drle(n, w, r, _u):
    """A ramp of RAMP[w] values (one delta run; a run each for Rle), then r runs of 2..127 equal values whose heads are w - 1 token
    bytes apart: such a run costs Rle w + 1 and DeltaRle w + 2."""
    ramp = np.arange(RAMP[w], dtype=np.int64) * (D_SHORT[w] + 1)
    heads = ramp[-1] + D_SHORT[w] * (1 + np.arange(r, dtype=np.int64))
    return np.concatenate([ramp, np.repeat(heads, _split(n - RAMP[w], r, 2, 127))])


# pair -> (builder, bytes of size[a] - size[b] per step of knob 0, per step of knob 1, smallest knob 1, first guess of knob 0)
FAMILY = {
    (DV, PAL): (_dv_pal, 1, 0, 0, lambda n, w: 2 + 200 * w),
    (DV, RLE): (_dv_rle, -3, 1, 0, lambda n, w: (n - 4) // 3),
    (DV, DRLE): (_dv_drle, 1, 0, 0, lambda n, w: 4),
    (PAL, RLE): (_pal_rle, lambda w: -(w + 1), -1, 0, lambda n, w: (n // 2 + 16 * w) // (w + 1)),
    (PAL, DRLE): (_pal_drle, -4, -1, 1, lambda n, w: (n // 2 + 16 * w) // 4),
    (RLE, DRLE): (_rle_drle, -1, 0, 0, lambda n, w: RAMP[w] * (w + 1) - w),
}


def _settle(build, a, b, want, k, ck, cu, ulo, sizes=None):
    """Knobs (k, u) at which sizes(build(k, u))[a] - [b] == want, given that a step of k moves it by ck and one of u by cu (+-1 or
    0): from a trial's sizes the knobs follow by division; a second round only where an edge of the column moved with them."""
    sizes = sizes or window_sizes
    u = ulo
    for _ in range(6):
        s = sizes(build(k, u))
        err = want - (s[a] - s[b])
        if err == 0:
            return k, u
        e = ck * k + cu * u + err
        for uu in range(ulo, ulo + abs(ck)):
            if (e - cu * uu) % ck == 0:
                k, u = (e - cu * uu) // ck, uu
                break
    raise AssertionError("the knobs did not settle")


def pair_column(pair, diff, n, ftype, sizes=None):
    """The family's column of n values with size[a] - size[b] == diff, as whole numbers that fit ftype (signed types: around 0)."""
    w = WIDTH_OF[ftype]
    build, ck, cu, ulo, k0 = FAMILY[pair]
    ck = ck(w) if callable(ck) else ck

    def column(k, u):
        v = build(n, w, k, u)
        return typed(v - (int(v.max()) // 2 if ftype in SIGNED else 0), ftype)
    k, u = _settle(column, pair[0], pair[1], diff, k0(n, w), ck, cu, ulo, sizes)
    return column(k, u)


def pair_cell(values):
    """(a, b, size[a] - size[b]) where the two smallest sizes of the window lie within one byte of each other and the two others
    at least 2 above the smaller; None elsewhere."""
    s = window_sizes(values)
    a, b = sorted(sorted(range(4), key=lambda m: (s[m], m))[:2])
    rest = [s[m] for m in range(4) if m not in (a, b)]
    if abs(s[a] - s[b]) <= 1 and min(rest) >= min(s[a], s[b]) + 2:
        return a, b, s[a] - s[b]
    return None


def length_class(values):
    n = len(values)
    return "mid" if 1025 < n < PROBE and n % 16 else "full" if n == PROBE else "beyond" if n > PROBE else "short"


# ---- values behind the window ------------------------------------------------------------------------------------------------

def _extremes(ftype):
    w = WIDTH_OF[ftype]
    if w == 8:
        return -(1 << 61), 1 << 61                      # 2^62 apart: a ten-byte delta that does not wrap
    ii = np.iinfo(NP[ftype])
    return int(ii.min) + 5, int(ii.max) - 5


def tail_for(mode, window, ftype, pair):
    """Values to lie behind the window that cost `mode` the least by far."""
    v = as_model(window)
    lo, hi = int(v.min()), int(v.max())
    if mode == DV:        # new values, one-byte deltas, none twice in a row
        t = hi + 1 + np.cumsum(1 + (np.arange(900) & 1))
    elif mode == PAL:     # hops among four values of the window, no delta twice in a row
        u = np.unique(v)
        t = np.tile([u[0], u[-1], u[1], u[-2]], 225)
    elif mode == RLE:     # 40 runs of 40 between two values far apart (the window's own where the Palette counts)
        a, b = (lo, hi) if PAL in pair else _extremes(ftype)
        t = np.repeat(np.tile([a, b], 20), 40)
    else:                 # one run of deltas
        t = hi + 1 + np.arange(900)
    return typed(t, ftype)


def beyond_cond(a, b, diff):
    def cond(values):
        s, t = window_sizes(values), whole_sizes(values)
        winner = M.select(s)
        loser = a + b - winner
        return (pair_cell(values[:PROBE]) == (a, b, diff) and len(values) > PROBE and len(values) <= CHUNK
                and M.select(t) == loser and t[winner] - t[loser] >= TAIL_MARGIN)
    return cond


# ---- rows ----------------------------------------------------------------------------------------------------------------------

ROWS = []
UNREACHED = []   # (family, cell, why)


def _add(name, family, ftype, values, cond):
    ROWS.append((name, family, ftype, values, cond))


def _pair_rows():
    for w in WIDTHS:
        for ci, (pair, diff) in enumerate(itertools.product(PAIRS, DIFFS)):
            a, b = pair
            tag = f"{MODE_NAMES[a]}_{MODE_NAMES[b]}_{'m0p'[diff + 1]}_w{w}"
            for cls, n in (("mid", MID_N[w] + 32 * ci), ("full", PROBE)):
                ftype = TYPES_OF[w][(ci + (cls == "full")) % 2]      # both types of a width in every class
                v = pair_column(pair, diff, n, ftype)
                _add(f"pair_{cls}_{tag}", "pair", ftype, v, lambda x, c=(a, b, diff), cls=cls: pair_cell(x) == c and length_class(x) == cls)
                if cls == "full":
                    loser = a + b - M.select(window_sizes(v))
                    _add(f"pair_beyond_{tag}", "pair", ftype, np.concatenate([v, tail_for(loser, v, ftype, pair)]), beyond_cond(a, b, diff))


def _tiny_rows():
    for ftype in (t for w in WIDTHS for t in TYPES_OF[w]):
        ii = np.iinfo(NP[ftype])
        vals = sorted({0, 1, 63, 64, int(ii.max), -1 if ftype in SIGNED else int(ii.max)})
        cast = np.array(vals, dtype=object).astype(NP[ftype])
        for n in (1, 2, 3, 4):
            for idx in itertools.product(range(len(vals)), repeat=n):
                _add(f"tiny_{ftype.name}_{'_'.join(map(str, idx))}", "tiny", ftype, cast[list(idx)], lambda x: len(window_sizes(x)) == 4)


# chunk 1 of a sums row: 300 values that cost one mode the least by far
def _second_chunk(mode, w):
    if mode == DV:
        return 7 + np.cumsum(1 + (np.arange(300) & 1))
    if mode == PAL:       # a walk by +-1, +-2 over few values (fewer for wider ones: the Palette is to win, not by everything)
        return np.array(_walk(0, 300, {2: 31, 4: 15, 8: 7}[w]))
    if mode == RLE:       # twenty runs of 15, twenty values
        return np.repeat(np.arange(20, dtype=np.int64) * (TOP[w] // 20), 15)
    return 11 + np.arange(300)


def sums_cond(a, b, diff):
    def cond(values):
        v, w = as_model(values), np.asarray(values).dtype.itemsize
        s0, s1, t = M.section_sizes(v[:CHUNK], w), M.section_sizes(v[CHUNK:], w), whole_sizes(values)
        clear = lambda s, m: all(s[o] >= s[m] + 16 for o in range(4) if o != m)
        rest = [t[m] for m in range(4) if m not in (a, b)]
        return (len(values) == CHUNK + 300 and clear(s0, a) and clear(s1, b) and t[a] - t[b] == diff
                and min(rest) >= min(t[a], t[b]) + 2)
    return cond


def _sums_rows():
    for w in WIDTHS:
        for ci, (pair, diff) in enumerate(itertools.product(PAIRS, DIFFS)):
            a, b = pair
            ftype = TYPES_OF[w][ci % 2]
            second = _second_chunk(b, w)
            name = f"sums_{MODE_NAMES[a]}_{MODE_NAMES[b]}_{'m0p'[diff + 1]}_w{w}"

            def sizes(first, second=second, ftype=ftype):
                return whole_sizes(np.concatenate([first, typed(second, ftype)]))
            try:
                first = pair_column(pair, diff, CHUNK, ftype, sizes)
                v = np.concatenate([first, typed(second, ftype)])
                assert sums_cond(a, b, diff)(v)
            except AssertionError:
                UNREACHED.append(("sums", name, "the family of the pair does not stretch to a chunk of 32768 values with the other "
                                  "two modes clear of the pair's sums"))
                continue
            _add(name, "sums", ftype, v, sums_cond(a, b, diff))


# ---- term triples ------------------------------------------------------------------------------------------------------------

TERMS = {}       # term -> (mode whose size the term is part of, {width: (tie, minus, plus) row names})
SAME_RAW = []    # (row under the unsigned type, row under the signed type): the same bytes, another mode


def _others_clear(s, m, rival):
    return min(s[o] for o in range(4) if o not in (m, rival)) >= min(s[m], s[rival]) + 2


def exact_cond(m, e, tie_values, extra=None):
    """Mode m is e bytes off the tie's size, the mode it ties with is where it was, the two others stay clear of both. The tie
    itself (e == 0): its two smallest sizes are equal and m is one of them."""
    tie = window_sizes(tie_values)
    low = sorted(range(4), key=lambda o: (tie[o], o))
    rival = low[1] if low[0] == m else low[0]

    def cond(values):
        s = window_sizes(values)
        return (m in low[:2] and tie[m] == tie[rival] and s[m] == tie[m] + e and s[rival] == tie[rival] and _others_clear(s, m, rival)
                and (extra is None or extra(values)))
    return cond


def near_cond(m, rival, e, extra=None):
    """size[m] - size[rival] == e, the two others clear of both."""
    def cond(values):
        s = window_sizes(values)
        return s[m] - s[rival] == e and _others_clear(s, m, rival) and (extra is None or extra(values))
    return cond


def _names(term, w):
    names = tuple(f"term_{term}_w{w}_{k}" for k in ("tie", "minus", "plus"))
    TERMS.setdefault(term, (None, {}))
    return names


def _exact_triple(term, m, ftype, tie, minus, plus, extra=None):
    """The neighbours differ from the tie in the one term."""
    w = WIDTH_OF[ftype]
    names = _names(term, w)
    for name, v, e in zip(names, (tie, minus, plus), (0, -1, 1)):
        _add(name, "term", ftype, typed(v, ftype), exact_cond(m, e, typed(tie, ftype), extra))
    TERMS[term] = (m, {**TERMS[term][1], w: names})


def _near_triple(term, m, rival, ftype, build, extra=None):
    """The term sits in every row of the triple; build(e) gives the column with size[m] - size[rival] == e."""
    w = WIDTH_OF[ftype]
    names = _names(term, w)
    for name, e in zip(names, (0, -1, 1)):
        _add(name, "term", ftype, build(e), near_cond(m, rival, e, extra))
    TERMS[term] = (m, {**TERMS[term][1], w: names})


WHERE = (("at_256", 192, TERM_N), ("at_1024", 960, TERM_N), ("at_end", None, TERM_N), ("behind_4096", None, PROBE))
BEHIND = 60


def _goes_on_behind(values):
    return len(values) == PROBE + BEHIND and values[PROBE - 1] == values[PROBE]


def _value_run_terms():
    """A run of 127 | 128 equal values (uvarint32_len of Rle's run length) in the Palette / Rle family: run A has 127 values in the
    tie and 128 in `plus`, run B 128 in the tie and 127 in `minus`; the run behind each gives or takes the value. Nothing else
    moves: the deltas keep their places' lengths, the zero runs of DeltaRle (126, 127) stay one byte. Where: A over the wave edge
    of 1024 threads (index 255 | 256), of 256 threads (1023 | 1024), A as the last run, ending at n, and A as the last run of a full
    window that goes on for 60 values behind it (its true length is 187 or 188)."""
    for where, front, n in WHERE:
        for w in WIDTHS:
            ftype = TYPES_OF[w][where != "at_256"]

            def lens(r, u, da=0, db=0):
                site_a, site_b = [127 + da, 30 - da], [128 + db, 30 - db]
                rest = [128] * u + _split(n - 315 - 128 * u - (front or 0), r - u - 4 - (front is not None), 2, 127)
                if front is None:
                    return site_b + rest + site_a[::-1]
                return [front] + site_a + site_b + rest
            shift = 8 * PAL_STEP[w] if ftype in SIGNED else 0

            def col(r, u, **kw):
                v = _pal_rle_lens(lens(r, u, **kw), w) - shift
                return typed(np.concatenate([v, np.full(BEHIND, v[-1])]) if n == PROBE else v, ftype)
            r, u = _settle(col, PAL, RLE, 0, (n // 2 + 16 * w) // (w + 1), -(w + 1), -1, 0)
            _exact_triple(f"value_run_127_128_{where}", RLE, ftype, col(r, u), col(r, u, db=-1), col(r, u, da=1),
                          _goes_on_behind if n == PROBE else None)


def _delta_run_terms():
    """The same for a run of 127 | 128 equal deltas (DeltaRle's run length) in a Rle / DeltaRle tie: two sites of two delta runs
    each, 127 + 20 and 128 + 20 deltas of the same token length; the edge between the two runs of a site moves by one. Every value
    is new, every value is a run of its own for Rle, and no token changes its length. Behind them runs of 2..127 equal values
    whose heads cost DeltaRle two bytes (k of them) or one byte (u of them) more than Rle."""
    c = 20
    for where, front, n in WHERE:
        for w in WIDTHS:
            ftype = TYPES_OF[w][where == "at_256"]
            d1, d2, d3, d4 = (D_SHORT[w] + i for i in (1, 2, 3, 4))

            def deltas(k, u, da=0, db=0):
                site_a, site_b = [d1] * (127 + da) + [d2] * (c - da), [d3] * (128 + db) + [d4] * (c - db)
                runs = []
                for i, l in enumerate(_split(n - (front or 0) - 2 * c - 255, k + u, 2, 127)):
                    runs += [D_LONG[w] if i < k else D_SHORT[w]] + [0] * (l - 1)
                if front is None:
                    return runs + site_b + site_a[::-1] + ([d1] * BEHIND if n == PROBE else [])
                return [D_SHORT[w]] + [0] * (front - 1) + site_a + site_b + runs
            shift = {2: 17500, 4: 1 << 29, 8: 1 << 58}[w] if ftype in SIGNED else 0
            col = lambda k, u, **kw: typed(np.cumsum(np.array(deltas(k, u, **kw), dtype=np.int64)) - shift, ftype)
            k, u = _settle(col, RLE, DRLE, 0, (2 * c + 255) * (w + 1) // 2, -2, -1, 0)
            extra = (lambda x: len(x) == PROBE + BEHIND and x[PROBE] - x[PROBE - 1] == x[PROBE - 1] - x[PROBE - 2]) if n == PROBE else None
            _exact_triple(f"delta_run_127_128_{where}", DRLE, ftype, col(k, u), col(k, u, db=-1), col(k, u, da=1), extra)


def _pal_rle_column(n, w, ftype, palette, e, order=None, lo=2, front=()):
    """Runs over the values of `palette` (in the order given, round and round, or heads order(number of runs)): Palette - Rle == e."""
    palette = np.asarray(palette, dtype=np.int64)
    bits = 0 if palette.size <= 1 else int(palette.size - 1).bit_length()

    def col(r, u):
        lens = list(front) + [128] * u + _split(n - sum(front) - 128 * u, r - u - len(front), lo, 127)
        idx = order(len(lens)) if order else np.arange(len(lens)) % palette.size
        return typed(np.repeat(palette[idx], lens), ftype)
    r, u = _settle(col, PAL, RLE, e, (3 + palette.size * w + (bits * n + 7) // 8 - 5) // (w + 1), -(w + 1), -1, 0)
    return col(r, u)


def _palette(count, w, ftype, step=None):
    step = step or PAL_STEP[w]
    return (np.arange(count, dtype=np.int64) - (count // 2 if ftype in SIGNED else 0)) * step


def _has_u(count):
    return lambda x: np.unique(x[:PROBE]).size == count


def _palette_terms():
    """U at 2^k | 2^k + 1 (palette_bits at its steps): near triples with exactly that many distinct values.
    U = 1: one value v, n times -- DeltaVarint = 1 + len(v) + n - 1 against Palette = 3 + w, the tie moved by n.
    U = 2 .. 17: runs over U values against Rle. U = 256, 257: the DeltaVarint / Palette family over U values.
    U = 2048, 2049: runs of 1..127 values against Rle, the heads going to and fro between the lower and the upper 1024 values (every
    delta as long as the type allows, or DeltaVarint would win; no delta twice in a row), for 2049 one more value in the 2100th run."""
    for w in WIDTHS:
        for ti, count in enumerate((1, 2, 3, 4, 5, 16, 17, 256, 257, 2048, 2049)):
            ftype = TYPES_OF[w][ti % 2]
            if count == 1:
                first = 70 if w < 8 else 1 << 30          # one token byte more where DeltaRle (5 + len + 3) has to stay above 3 + w
                f = 2 if w < 8 else 5
                _near_triple("palette_u_1", DV, PAL, ftype, lambda e: typed(np.full(3 + w - f + e, first), ftype), _has_u(1))
            elif count <= 17:
                _near_triple(f"palette_u_{count}", PAL, RLE, ftype,
                             lambda e: _pal_rle_column(TERM_N, w, ftype, _palette(count, w, ftype), e), _has_u(count))
            elif count <= 257:
                def build(e):
                    col = lambda z, _u: typed(_dv_pal(TERM_N, w, z, 0, count) - (550 if ftype in SIGNED else 0), ftype)
                    z, _u = _settle(col, DV, PAL, -e, 2 + count * w + (TERM_N // 8 if count == 257 else 0), 1, 0, 0)
                    return col(z, 0)
                _near_triple(f"palette_u_{count}", PAL, DV, ftype, build, _has_u(count))
            else:
                ftype = TYPES_OF[w][0]                     # the values fill the unsigned type
                step = {2: 31, 4: 1 << 20, 8: 1 << 50}[w]

                def order(runs):
                    r = np.arange(runs, dtype=np.int64)
                    idx = (r // 2) % 1024 + 1024 * (r % 2)
                    if count == 2049:
                        idx[2100] = 2048
                    return idx
                _near_triple(f"palette_u_{count}", PAL, RLE, ftype,
                             lambda e: _pal_rle_column(TERM_N, w, ftype, np.arange(count, dtype=np.int64) * step, e, order, lo=1), _has_u(count))


def _all_ones_terms():
    """The all-ones value as one of 16, under the unsigned and the signed type of every width: the hash table of the wide keys keeps
    it on the side (its free-slot mark)."""
    for w in WIDTHS:
        for ftype in TYPES_OF[w]:
            ones = -1 if ftype in SIGNED or w == 8 else (1 << (8 * w)) - 1
            pal = np.concatenate([[ones], np.arange(15, dtype=np.int64) * PAL_STEP[w] + 3])
            _near_triple("all_ones_value" + ("_signed" if ftype in SIGNED else ""), PAL, RLE, ftype,
                         lambda e: _pal_rle_column(TERM_N, w, ftype, pal, e),
                         lambda x: np.unique(x).size == 16 and (x.view(np.uint8) == 0xFF).reshape(-1, x.dtype.itemsize).all(axis=1).any())


def _index_byte_terms():
    """(bits * n + 7) >> 3 with bits * n congruent to 0 and to 1 modulo 8: 8 values (3 bits), n = 4088 and n = 4091."""
    for n, rem in ((4088, 0), (4091, 1)):
        assert (3 * n) % 8 == rem and n % 16
        for w in WIDTHS:
            ftype = TYPES_OF[w][rem]
            _near_triple(f"index_bytes_mod8_{rem}", PAL, RLE, ftype, lambda e: _pal_rle_column(n, w, ftype, _palette(8, w, ftype), e), _has_u(8))


def _cross_wave_terms():
    """A run whose head is the last value of a thread in both geometries (index 15) and whose next head lies 2100 values on: more
    than two waves of 1024 values, more than eight of 256. The run length comes from the cross-wave loop of
    block_suffix_min_exclusive alone."""
    for w in WIDTHS:
        ftype = TYPES_OF[w][1]
        _near_triple("run_over_two_waves", RLE, PAL, ftype, lambda e: _pal_rle_column(TERM_N, w, ftype, _palette(16, w, ftype), -e, front=(15, 2100)),
                     lambda x: x[14] != x[15] and (x[15:2115] == x[15]).all() and x[2115] != x[15])


def _dv_rle_column(n, w, ftype, prefix, e, top=None, exact=False):
    """The DeltaVarint / Rle family behind run heads given in `prefix`: DeltaVarint - Rle == e."""
    top = top or TOP[w]

    def col(r, u):
        deltas = [D_SHORT[w]] * (r - len(prefix))
        deltas[:u] = [D_LONG[w]] * u
        heads = np.concatenate([np.array(prefix, dtype=np.int64), prefix[-1] + _bounce(deltas, top - 2 * D_LONG[w])[1:]])
        return typed(np.repeat(heads, _split(n, r, 2, 127)), ftype)
    r, u = _settle(col, DV, RLE, e, (n - 4) // 3, -3, 1, 0)
    return (lambda p: (prefix.__setitem__(slice(None), p), col(r, u))[1]) if exact else col(r, u)


def _first_token_terms():
    """The first value's own token (values[-1] = 0): 63 | 64 | 8192 as the first value, one, two and three bytes; the second head
    is 20000, three bytes away from each of them."""
    for w in WIDTHS:
        ftype = {2: F.UINT16, 4: F.INT32, 8: F.INT64}[w]
        prefix = [64, 20000]
        at = _dv_rle_column(TERM_N, w, ftype, prefix, 0, exact=True)
        _exact_triple("first_value_token", DV, ftype, at([64, 20000]), at([63, 20000]), at([8192, 20000]))


def _varint_step_terms():
    """A delta either side of each length step of varint64_len that the width can hold, 2^(7k - 1) for k = 1 .. (2, 4, 9), rising and
    falling: two spikes c, c +- d, c -+ 5 in front of the DeltaVarint / Rle family. Spike A has d = step - 1 in the tie and the
    step in `plus`, spike B the step in the tie and step - 1 in `minus`; the way back (d + 5) keeps its length."""
    for w in WIDTHS:
        for k in range(1, {2: 2, 4: 4, 8: 9}[w] + 1):
            step = 1 << (7 * k - 1)
            for sign in (1, -1):
                ftype = TYPES_OF[w][0] if w == 2 else TYPES_OF[w][1] if w == 4 else TYPES_OF[w][k % 2]
                c = 100 if sign > 0 else step + 100
                heads = lambda da, db: [c, c + sign * da, c - sign * 5, c - sign * 5 + sign * db, c - sign * 10]
                prefix = heads(step - 1, step)
                top = TOP[w] if w < 8 or sign > 0 else (1 << 60)
                at = _dv_rle_column(TERM_N, w, ftype, prefix, 0, top, exact=True)
                _exact_triple(f"varint_step_{k}_{'rising' if sign > 0 else 'falling'}", DV, ftype, at(heads(step - 1, step)),
                              at(heads(step - 1, step - 1)), at(heads(step, step)))


def _int64_terms():
    """64-bit deltas that wrap: -2^62 -> 2^62 is 2^63 = INT64_MIN, whose zig-zag + 1 wraps to 0 and costs ONE byte; one value
    further apart and the delta is -(2^63 - 7), ten bytes."""
    lo = np.iinfo(np.int64).min
    for ti, (term, a) in enumerate((("int64_min_delta", -(1 << 62)), ("int64_wrap_around_delta", -(1 << 62) - 7))):
        ftype = TYPES_OF[8][ti]
        want = lo if ti == 0 else -((1 << 63) - 7)

        def has(x, want=want):
            v = as_model(x)
            return bool(((v[1:] - v[:-1]) == want).any())
        _near_triple(term, DV, RLE, ftype, lambda e: _dv_rle_column(TERM_N, 8, ftype, [100, a, 1 << 62, 300], e), has)


def _same_raw_rows():
    """One raw 16-bit column either side of 0x8000: small deltas as UINT16 (a DeltaVarint / Palette tie, DeltaVarint commits),
    deltas of three bytes as INT16 (Palette commits)."""
    v = pair_column((DV, PAL), 0, TERM_N, F.UINT16, lambda x: window_sizes(x + np.uint16(0x8000 - 500))) + np.uint16(0x8000 - 500)
    _add("same_raw_16_as_uint16", "term", F.UINT16, v, lambda x: pair_cell(x) == (DV, PAL, 0))
    _add("same_raw_16_as_int16", "term", F.INT16, v.view(np.int16),
         lambda x: M.select(window_sizes(x)) == PAL and (x < 0).any() and (x > 0).any())
    SAME_RAW.append(("same_raw_16_as_uint16", "same_raw_16_as_int16"))


def _build():
    _pair_rows()
    _value_run_terms()
    _delta_run_terms()
    _palette_terms()
    _all_ones_terms()
    _index_byte_terms()
    _cross_wave_terms()
    _first_token_terms()
    _varint_step_terms()
    _int64_terms()
    _same_raw_rows()
    _tiny_rows()
    _sums_rows()


_build()
BY_NAME = {r[0]: r for r in ROWS}

# ---- what is not here ---------------------------------------------------------------------------------------------------------
# UNREACHED holds the cells a builder above gave up on; there are none: all 18 (pair, diff) cells are built at every width in the
# mid, full and beyond classes, and all 18 sums cells at every width. One term of the list has no row at any width:
NO_ROW = [("palette_u_4096", "U == n == 4096 (12 index bits): Palette = 3 + 4096 w + 6144 lies above Rle <= 5 + 4096 (w + 1) by at least "
           "2042 bytes whatever the values, so Palette is never within reach of the smallest size and no bit count it takes there can "
           "change a verdict; U = 2049 (12 bits as well) is the largest palette with a tie, and it has its triple")]


def rows(*families):
    return [r for r in ROWS if r[1] in families]
