"""The inputs of the tests of ZSTD frames WITH sequences (tests/test_zstd_seq_rules.py, test_zstd_seq_walk_cpu.py,
test_gpu_zstd_seq_decode.py). It extends tests/zstd_decode_cases.py; the verdicts are tests/zstd_seq_rules.py's.
  a  grid_frames()      frames built by hand with all three tables in RLE mode (or Repeat of such a table): the bit stream then
                        holds extra bits only, so no FSE encoder is needed. Every sequence of a block has the same three codes;
                        build() cuts a list of sequences into blocks where the codes change.
  b  libzstd_frames()   the system libzstd over sources x levels 1, 3 and the small-block parameters
     lidar_frames()     ... and over one full stage-1 chunk of two lidar schemas (they need the oracle's encoder)
  c  damaged_base(i)    single-byte changes of the bytes the new walk reads beyond the old one, truncations, random damage,
                        flips in the last 8 bytes of the bit stream
Entries are (name, frame, capacity, payload or None); payload is what went into the compressor, or for (a) what expand()
below makes of the sequences -- never the model's output. None: the rules must not say OK."""
import functools

import numpy as np

import zstd_decode_cases as K
import zstd_lit_model as M
import zstd_seq_rules as S

LEVEL3 = ((K.C_LEVEL, 3),)
# Frames of libzstd_frames() that libzstd accepts and the rules hand to the host, by name and rule: with 1 KiB blocks 40000
# constant bytes are one block with a match and 39 RLE blocks of 4 bytes each, 176 bytes in all: 40 blocks against a record
# limit of 4 + 176 / 16 = 15 (a record per 4 source bytes would be needed, and the workspace is sized by that ratio).
LIBZSTD_HOST = {"constant/small_blocks/40000": "record limit"}


def ring():
    """the bytes of k_zstd_seq_exec's LDS ring, from the library itself (a host function: no GPU)"""
    from cloudini_amd import native
    return int(native.zstd_seq_ring())


def _code(value, base, bits):
    for c in range(len(base) - 1, -1, -1):
        if base[c] <= value:
            assert value - base[c] < (1 << bits[c]), value
            return c
    raise AssertionError(value)


def codes_of(ll, ml, ofv):
    return _code(ll, S.LL_BASE, S.LL_BITS), ofv.bit_length() - 1, _code(ml, S.ML_BASE, S.ML_BITS)


def expand(items, prefix=b""):
    """items: (literal bytes, ml, offset value) per sequence, a "|" forces a new block, an entry of bytes: literals without a
    sequence (the end of a block); prefix: content of blocks in front -> the content, or None when a match reaches in front of
    it or `rep1 - 1` gives 0"""
    out = bytearray(prefix)
    rep = [1, 4, 8]
    for it in items:
        if it == "|":
            continue
        if isinstance(it, (bytes, bytearray)):
            out += it
            continue
        lit, ml, ofv = it
        out += lit
        if ofv > 3:
            off = ofv - 3
            rep = [off, rep[0], rep[1]]
        else:
            idx = ofv - 1 + (len(lit) == 0)
            off = (rep[0], rep[1], rep[2], rep[0] - 1)[idx]
            if off == 0:
                return None
            rep = rep if idx == 0 else [off, rep[0], rep[2]] if idx == 1 else [off, rep[0], rep[1]]
        if off > len(out):
            return None
        for _ in range(ml):
            out.append(out[-off])
    return bytes(out)


def _lit_section(lits: bytes, how):
    n = len(lits)
    if isinstance(how, str) and how == "raw":
        return K._short_header(0, n, 0 if n < 32 else 1 if n < 4096 else 3) + lits
    if isinstance(how, str) and how == "rle":
        assert n and lits == lits[:1] * n
        return K._short_header(1, n, 0 if n < 32 else 1 if n < 4096 else 3) + lits[:1]
    data = np.frombuffer(lits, np.uint8)
    four = n >= 256
    if isinstance(how, str) and how == "huf":
        desc, body, _lens = K.huf_pieces(data, four)
        return K.lit_header(2, n, len(desc) + len(body), four) + desc + body
    _desc, body, _lens = K.huf_pieces(data, four, how)               # treeless: `how` is the lengths of the earlier block
    return K.lit_header(3, n, len(body), four) + body


def seq_block(seqs, trailing: bytes, last, *, lit="raw", repeat=(False, False, False), nb_form=None, modes_low=0):
    """one Compressed block: seqs [(literal bytes, ml, offset value)] that share their three codes; RLE tables, or Repeat"""
    lits = b"".join(s[0] for s in seqs) + trailing
    cs = {codes_of(len(l), ml, ofv) for l, ml, ofv in seqs}
    assert len(cs) == 1, cs
    llc, ofc, mlc = cs.pop()
    nb = len(seqs)
    form = nb_form or (1 if nb < 128 else 2 if nb < 0x7F00 else 3)
    head = bytes([nb]) if form == 1 else bytes([128 + (nb >> 8), nb & 255]) if form == 2 else b"\xff" + (nb - 0x7F00).to_bytes(2, "little")
    modes = [S.REPEAT if r else S.MODE_RLE for r in repeat]
    head += bytes([(modes[0] << 6) | (modes[1] << 4) | (modes[2] << 2) | modes_low])
    head += b"".join(bytes([c]) for c, r in zip((llc, ofc, mlc), repeat) if not r)
    acc, nbits = 0, 0
    for l, ml, ofv in reversed(seqs):                   # written in the reverse of the reading order: OF, ML, LL per sequence
        for v, k in ((len(l) - S.LL_BASE[llc], S.LL_BITS[llc]), (ml - S.ML_BASE[mlc], S.ML_BITS[mlc]), (ofv - (1 << ofc), ofc)):
            acc |= v << nbits
            nbits += k
    acc |= 1 << nbits
    sec = _lit_section(lits, lit) + head + acc.to_bytes(nbits // 8 + 1, "little")
    return M.block_header(last, 2, len(sec)) + sec


def build(items, *, use_repeat=False, first_repeat=(False, False, False), lit="raw", pre=b"", pre_payload=b"", **kw):
    """-> (frame, payload): items as for expand(); a new block starts where the codes change or a "|" stands.
    pre: blocks in front (their content: pre_payload)"""
    blocks, cur, prev_codes = [], [], None
    trailing = b""
    items = list(items)
    if items and isinstance(items[-1], (bytes, bytearray)):
        trailing = bytes(items.pop())
    groups = []
    for it in items:
        if it == "|" or (cur and codes_of(len(it[0]), it[1], it[2]) != codes_of(len(cur[0][0]), cur[0][1], cur[0][2])):
            if cur:
                groups.append(cur)
            cur = []
        if it != "|":
            cur.append(it)
    if cur:
        groups.append(cur)
    for g, seqs in enumerate(groups):
        c = codes_of(len(seqs[0][0]), seqs[0][1], seqs[0][2])
        rep = tuple(use_repeat and prev_codes[t] == c[t] for t in range(3)) if prev_codes else tuple(first_repeat)
        blocks.append(seq_block(seqs, trailing if g == len(groups) - 1 else b"", g == len(groups) - 1, lit=lit, repeat=rep, **kw))
        prev_codes = c
    payload = expand(items + [trailing], pre_payload)
    return K.frame_header(len(payload) if payload is not None else 0, single=False, fcs_bytes=4) + pre + b"".join(blocks), payload


def one_seq_block(lit: bytes, trailing: bytes, last, modes, descs, tables, want):
    """one Compressed block (Raw literals) with ONE sequence: its bit stream is the three initial states and the extra bits, so
    no FSE encoder is needed. modes: Predefined, FSE or Repeat per table; descs: the description bytes of the FSE ones; tables:
    [(table, log)] in use (tests/zstd_seq_rules.py fse_table); want(t, symbol) -> bool picks the state of table t.
    -> (block, (literal bytes, ml, offset value))"""
    st = [next(k for k, e in enumerate(tab) if want(t, e[0])) for t, (tab, _log) in enumerate(tables)]
    llc, ofc, mlc = (tables[t][0][st[t]][0] for t in range(3))
    ll, ml, ofv = S.LL_BASE[llc], S.ML_BASE[mlc], 1 << ofc                  # every extra bit 0
    assert ll == len(lit)
    acc, nbits = 0, S.LL_BITS[llc] + S.ML_BITS[mlc] + ofc                    # the extra bits, then ML, OF, LL states on top
    for t in (S.ML, S.OF, S.LL):
        acc |= st[t] << nbits
        nbits += tables[t][1]
    acc |= 1 << nbits
    head = bytes([1, (modes[0] << 6) | (modes[1] << 4) | (modes[2] << 2)]) + b"".join(descs)
    sec = _lit_section(lit + trailing, "raw") + head + acc.to_bytes(nbits // 8 + 1, "little")
    return M.block_header(last, 2, len(sec)) + sec, (lit, ml, ofv)


def chain_block(lits, trailing: bytes, last, modes, descs, tables, wants):
    """one Compressed block (Raw literals) with len(wants) sequences under Predefined or FSE tables, built forwards as the decoder
    reads it, so no FSE encoder is needed: the initial states are free, and a state update is baseline + the bits read, so
    the bits choose the next state among those the entry reaches. wants[k](t, symbol) -> bool picks sequence k's symbols (codes
    without extra bits: every extra bit is 0); the LAST reachable state that fits is taken, so the update bits are not all 0
    and the order LL, ML, OF of the updates shows. -> (block, [(literal bytes, ml, offset value)])"""
    reads, seqs = [], []                                  # (value, bits) in the order the decoder reads them
    st = [None] * 3
    for k, want in enumerate(wants):
        for t in ((S.LL, S.OF, S.ML) if k == 0 else (S.LL, S.ML, S.OF)):
            tab, log = tables[t]
            if k == 0:
                st[t] = max(u for u, e in enumerate(tab) if want(t, e[0]))
                reads.append((st[t], log))
            else:
                _sym, nb, base = tab[st[t]]
                v = max(v for v in range(1 << nb) if want(t, tab[base + v][0]))
                reads.append((v, nb))
                st[t] = base + v
        llc, ofc, mlc = (tables[t][0][st[t]][0] for t in range(3))
        assert S.LL_BITS[llc] == 0 and S.ML_BITS[mlc] == 0 and S.LL_BASE[llc] == len(lits[k]), (k, llc, len(lits[k]))
        reads.append((0, ofc))
        seqs.append((lits[k], S.ML_BASE[mlc], 1 << ofc))
    acc, nbits = 0, 0
    for v, n in reversed(reads):
        acc |= v << nbits
        nbits += n
    acc |= 1 << nbits
    head = bytes([len(wants), (modes[0] << 6) | (modes[1] << 4) | (modes[2] << 2)]) + b"".join(descs)
    sec = _lit_section(b"".join(lits) + trailing, "raw") + head + acc.to_bytes(nbits // 8 + 1, "little")
    return M.block_header(last, 2, len(sec)) + sec, seqs


def chains_of_tables():
    """one-block frames of three sequences under Predefined and under FSE_Compressed tables (the descriptions are those of a
    block libzstd wrote): the state updates of the constructed grid. -> [(name, frame, capacity, payload)]"""
    out = []
    for name, mode, tables, d in _table_sets():
        # (literal lengths 8..15, then 1..7, then any below 16; offsets that stay inside what is produced: codes 2..3 are the
        # offsets 1..5, code 4 is 13, codes 0 and 1 the repeat offsets)
        wants = [lambda t, sym: (8 <= sym <= 15) if t == S.LL else (2 <= sym <= 3) if t == S.OF else sym < 32,
                 lambda t, sym: (1 <= sym <= 7) if t == S.LL else (2 <= sym <= 4) if t == S.OF else (0 < sym < 32),
                 lambda t, sym: sym <= 15 if t == S.LL else sym <= 4 if t == S.OF else sym < 20]
        # (the literal lengths follow from the states chosen: build once to learn them, then with literals of those lengths)
        probe = _chain_lengths(tables, wants)
        lits = [_rnd(20, 41 + k)[:n] for k, n in enumerate(probe)]
        blk, seqs = chain_block(lits, b"tail", True, [mode] * 3, d, tables, wants)
        payload = expand(seqs + [b"tail"])
        assert payload is not None, name
        out.append((f"chain/{name}", K.frame_header(len(payload), single=False, fcs_bytes=4) + blk, len(payload), payload))
    return out


def _chain_lengths(tables, wants):
    """the literal lengths chain_block's choice of states gives"""
    st, out = [None] * 3, []
    for k, want in enumerate(wants):
        for t in range(3):
            tab, _log = tables[t]
            if k == 0:
                st[t] = max(u for u, e in enumerate(tab) if want(t, e[0]))
            else:
                _sym, nb, base = tab[st[t]]
                st[t] = base + max(v for v in range(1 << nb) if want(t, tab[base + v][0]))
        out.append(S.LL_BASE[tables[0][0][st[0]][0]])
    return out


def _table_sets():
    """-> [(name, mode, [(table, log)] x 3, description bytes x 3)]: the predefined tables, and those of a block libzstd wrote"""
    pre = [(S.fse_table(S.DEFAULT_NORM[t], S.DEFAULT_LOG[t]), S.DEFAULT_LOG[t]) for t in range(3)]
    src = next(f for n, f, _c, _p in libzstd_frames() if n == "zipf/level3/5000")
    blk = next(b for b in S.walk(src, 1 << 20, all_blocks=True)[1] if b["seq"] and b["seq"]["modes"] == [S.FSE] * 3)
    fse = [(S.fse_table(*blk["seq"]["norm"][t]), blk["seq"]["norm"][t][1]) for t in range(3)]
    descs = [src[a:a + n] for a, n in blk["seq"]["tab"]]
    return [("predefined", S.PREDEFINED, pre, [b""] * 3), ("fse", S.FSE, fse, descs)]


def repeat_of_tables():
    """two-block frames whose second block says Repeat for all three tables, behind a block with Predefined tables and behind
    one with FSE_Compressed tables (the descriptions are those of a block libzstd wrote): libzstd writes no Repeat mode over
    these sources. -> [(name, frame, capacity, payload)]"""
    out = []
    for name, mode, tables, d in _table_sets():
        # literal lengths 8..15 (a code is the length), an offset inside the literals, any match length without extra bits
        want1 = lambda t, sym: (8 <= sym <= 15) if t == S.LL else (3 <= sym <= 5) if t == S.OF else sym < 32
        want2 = lambda t, sym: (4 <= sym <= 7) if t == S.LL else (2 <= sym <= 6) if t == S.OF else (sym < 32 and sym != 0)
        ll1 = S.LL_BASE[next(e[0] for e in tables[0][0] if want1(S.LL, e[0]))]
        ll2 = S.LL_BASE[next(e[0] for e in tables[0][0] if want2(S.LL, e[0]))]
        b1, s1 = one_seq_block(_rnd(40, 31)[:ll1], _rnd(70, 32), False, [mode] * 3, d, tables, want1)
        b2, s2 = one_seq_block(_rnd(40, 33)[:ll2], b"end", True, [S.REPEAT] * 3, [b""] * 3, tables, want2)
        items = [s1, _rnd(70, 32), s2, b"end"]
        payload = expand(items)
        assert payload is not None
        out.append((f"repeat_of/{name}", K.frame_header(len(payload), single=False, fcs_bytes=4) + b1 + b2, len(payload), payload))
    return out


def _rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def grid_frames():
    """-> [(name, frame, capacity, payload or None)]"""
    out = []

    def add(name, items, payload_ok=True, **kw):
        frame, payload = build(items, **kw)
        assert (payload is not None) == payload_ok, name
        cap = len(payload) if payload is not None else 1 << 16
        out.append((name, frame, cap, payload))
    # match length x offset behind 80 + r literals: the match's destination at residue (80 + r) % 16
    for ml in (3, 4, 15, 16, 17, 63, 64, 65):
        for off in (1, 2, 3, 15, 16, 63, 64, 65):
            r = (3 * ml + off) % 16
            add(f"match/ml{ml}/off{off}/r{r}", [(_rnd(80 + r, ml * 100 + off), ml, off + 3), _rnd(5, 1)])
    for off in (1, 65):
        add(f"match/ml70000/off{off}", [(_rnd(80, 7), 70000, off + 3), b"xyz"])   # (ML code 52: baseline 65539)
    for ml, off in ((17, 3), (65, 64), (64, 16), (40, 100)):
        for r in range(16):
            add(f"align/ml{ml}/off{off}/r{r}", [(_rnd(112 + r, r), ml, off + 3), _rnd(3, 2)])
    add("reach/all", [(_rnd(100, 3), 20, 100 + 3)])
    add("reach/one_more", [(_rnd(100, 3), 20, 101 + 3)], payload_ok=False)
    for ll in (0, 1, 15, 16, 17):
        add(f"ll/{ll}", [(_rnd(20, 4), 5, 7 + 3), (_rnd(ll, 5), 6, 11 + 3), _rnd(2, 6)])
    hist = [(_rnd(30, 8), 4, 5 + 3), (_rnd(3, 9), 4, 9 + 3), (_rnd(3, 10), 4, 14 + 3)]       # rep = 14, 9, 5
    for ofv in (1, 2, 3):
        for ll in (0, 2):
            add(f"rep/{ofv}/ll{ll}", hist + [(_rnd(ll, 11), 7, ofv)] + [b"end"])
    add("rep/three_in_a_row", hist + [(b"", 5, 1), (b"ab", 6, 2), (b"", 7, 3), (b"c", 4, 1)] + [b"end"])
    add("rep/all_values_twice", hist + [(b"q", 5, 3), (b"", 5, 2), (b"r", 5, 2), (b"", 5, 1), (b"", 9, 3), (b"s", 3, 1)])
    add("host/rep1_minus_1_is_0", [(_rnd(10, 12), 4, 1 + 3), (b"", 4, 3)], payload_ok=False)
    # two blocks: the history carries over, the second block's match reads the first block's bytes
    add("two_blocks/history", [(_rnd(40, 13), 6, 7 + 3), "|", (_rnd(40, 14), 9, 1), (b"", 5, 30 + 3), b"t"])
    add("two_blocks/repeat_modes", [(_rnd(40, 13), 6, 7 + 3), "|", (_rnd(40, 15), 6, 6 + 3), b"t"], use_repeat=True)
    add("two_blocks/repeat_some", [(_rnd(40, 13), 6, 7 + 3), "|", (_rnd(40, 15), 9, 6 + 3), "|", (_rnd(8, 16), 9, 40 + 3)], use_repeat=True)
    add("corrupt/repeat_without_table", [(_rnd(40, 13), 6, 7 + 3)], payload_ok=True, first_repeat=(True, False, False))
    out.append(out.pop()[:3] + (None,))               # (expand() knows no modes: the frame's first block says Repeat for LL)
    f, p = build([(_rnd(40, 13), 6, 7 + 3)])
    q = 10 + 3 + 2 + 40                                # frame header, block header, literals header (12 bits), the literals
    assert f[q] == 1 and f[q + 1] == 0x54              # the count, the modes byte; then the three RLE symbols
    out.append(("host/reserved_bits", f[:q + 1] + bytes([0x55]) + f[q + 2:], len(p), None))
    out.append(("corrupt/rle_symbol_36", f[:q + 2] + bytes([36]) + f[q + 3:], len(p), None))
    # count forms
    add("count/one_in_two_bytes", [(b"ab", 3, 1 + 3), b"z"], nb_form=2)
    add("count/128", [(b"a", 3, 1 + 3)] * 128 + [b"z"])
    add("count/three_bytes", [(b"a", 3, 1 + 3)] * 0x7F00 + [b"z"])
    # (a count of 256 in two bytes, then the same frame with those bytes saying 0)
    add("host/count_zero_long_form", [(b"a", 3, 1 + 3)] * 256 + [b"z"], payload_ok=True)
    name, f256, cap, _p = out.pop()
    i = f256.index(bytes([129, 0]))
    out.append((name, f256[:i] + bytes([128, 0]) + f256[i + 2:], cap, None))
    # literals of every kind under a sequence block; Raw, RLE and literal-only blocks around sequence blocks
    a = K.G.skewed(700, 11)
    b = K.G.skewed(300, 12, top=12)
    lens_a = M.code_lengths(np.bincount(a, minlength=256))
    add("literals/huf", [(a.tobytes()[:400], 30, 200 + 3), a.tobytes()[400:]], lit="huf")
    add("literals/rle", [(b"\x07" * 50, 9, 50 + 3), b"\x07" * 20], lit="rle")
    two = [(a.tobytes()[:400], 30, 200 + 3), a.tobytes()[400:], (b.tobytes()[:100], 12, 500 + 3), b.tobytes()[100:]]
    first = seq_block(two[:1], two[1], False, lit="huf")
    second = seq_block(two[2:3], two[3], True, lit=lens_a)
    p = expand(two)
    out.append(("literals/treeless", K.frame_header(len(p), single=False) + first + second, len(p), p))
    pre = (M.block_header(False, 0, 30) + a[:30].tobytes() + M.block_header(False, 1, 40) + b"\x05" + M.block_header(False, 0, 0) +
           K.huf_block(a, False, True))
    add("mixed/raw_rle_literal_only_then_sequences", [(_rnd(10, 17), 20, 770 + 3), (b"", 8, 2), b"tail"], pre=pre,
        pre_payload=a[:30].tobytes() + b"\x05" * 40 + a.tobytes())
    # the ring and global memory: the output exceeds the kernel's ring, and a match of one step (60 bytes) or several (200) reaches
    # back to the ring's last byte (lane 0 of a step reads the byte `offset` back: in the ring up to offset == ring), one byte
    # further (lane 0 from global memory, the others from the ring), half a step further (straddling), a whole step further
    # (all from global memory); a periodic match longer than the ring whose period lies outside it
    R = ring()
    big = _rnd(R + 3000, 18)
    for name, off in (("inside", R), ("outside_by_one", R + 1), ("straddling", R + 32), ("outside", R + 64)):
        for ml in (60, 200):
            add(f"ring/{name}/ml{ml}", [(big[:R + 2000], 40, 17 + 3), "|", (big[R + 2000:R + 2500], ml, off + 3), (b"", 50, R + 1900 + 3), big[R + 2500:]])
    add("ring/periodic_outside", [(big[:R + 2000], 40, 17 + 3), "|", (big[R + 2000:R + 2500], R + 9000, R + 5 + 3), big[R + 2500:]])
    add("ring/second_block", [(_rnd(120000, 19), 300, 110000 + 3), "|", (_rnd(70000, 20), 3000, 180000 + 3), b"e"])
    out.extend(repeat_of_tables())
    out.extend(chains_of_tables())
    # capacity
    name, f, cap, p = out[0]
    out.append(("capacity/one_short", f, cap - 1, None))
    return out


HOST_BY_RULE = ("host/rep1_minus_1_is_0", "host/reserved_bits", "host/count_zero_long_form")


@functools.lru_cache(None)
def libzstd_frames():
    out = []
    src = K.sources()
    for sname in ("geometric", "zipf", "constant", "random"):
        for pname, params in (("level1", K.LEVEL1), ("level3", LEVEL3), ("small_blocks", K.SMALL_BLOCKS)):
            for n in (200, 5000, 40000) + ((300000,) if pname != "small_blocks" else ()):
                p = src[sname][:n]
                out.append((f"{sname}/{pname}/{n}", K.libzstd_compress(p, params), n, p))
    text = (b"the quick brown fox jumps over the lazy dog; " * 9000)[:300000]
    mix = bytearray(text)
    rs = np.random.default_rng(5)
    for at in rs.integers(0, len(mix), 3000):
        mix[int(at)] = int(rs.integers(0, 256))
    for pname, params in (("level1", K.LEVEL1), ("level3", LEVEL3)):
        out.append((f"text/{pname}", K.libzstd_compress(bytes(mix), params), len(mix), bytes(mix)))
    far = _rnd(150000, 21)
    far2 = far + far[:100000]                             # matches 150000 bytes back
    out.append(("far_repeat/level3", K.libzstd_compress(far2, LEVEL3 + ((K.C_WINDOW_LOG, 18),)), len(far2), far2))
    return out


def lidar_frames(oracle):
    """one full 32768-point chunk of two lidar schemas, stage 1 by the oracle, stage 2 by libzstd level 1"""
    from cloudini_amd import synth
    out = []
    for name, make in (("lidar_xyzi", synth.lidar_xyzi), ("velodyne_xyzir", synth.velodyne_xyzir)):
        info, data = make(32768)
        s1 = np.ascontiguousarray(oracle.encode_stage1(info, np.ascontiguousarray(data).view(np.uint8).reshape(-1))).view(np.uint8).reshape(-1)
        n = int.from_bytes(s1[:4].tobytes(), "little")
        p = s1[4:4 + n].tobytes()
        out.append((f"{name}/level1", K.libzstd_compress(p, K.LEVEL1), len(p), p))
    return out


# ---- c -----------------------------------------------------------------------------------------------------------------------------
MAX_NEW_POSITIONS = 24
DAMAGE_NAMES = ("ll/16", "rep/three_in_a_row", "two_blocks/repeat_some", "literals/treeless", "match/ml65/off3/r6")
DAMAGE_LIB = ("geometric/level1/200", "zipf/level3/5000", "geometric/small_blocks/5000")


@functools.lru_cache(None)
def damage_bases():
    g = {n: (f, c) for n, f, c, _p in grid_frames()}
    l = {n: (f, c) for n, f, c, _p in libzstd_frames()}
    return [g[n] for n in DAMAGE_NAMES] + [l[n] for n in DAMAGE_LIB]


def new_positions(frame: bytes):
    """the bytes the new walk reads beyond the old one -- counts, modes bytes, table descriptions, RLE bytes --, the first
    MAX_NEW_POSITIONS of them in frame order"""
    note = {}
    S.walk(frame, 1 << 30, all_blocks=True, note=note)
    pos = sorted({at for a, b in note.get("seq_headers", []) for at in range(a, min(b, len(frame)))})
    return pos[:MAX_NEW_POSITIONS]


def bit_stream_tail(frame: bytes):
    """the last 8 bytes of the first bit stream"""
    _v, blocks, _s = S.walk(frame, 1 << 30, all_blocks=True)
    for blk in blocks:
        if blk["seq"] is not None:
            a, b = blk["seq"]["bits"]
            return list(range(max(a, b - 8), b))
    return []


@functools.lru_cache(None)
def damaged_base(i: int):
    """-> [(name, frame, capacity)]"""
    f, cap = damage_bases()[i]
    out = []
    for at in new_positions(f):
        for delta in range(1, 256):
            g = bytearray(f)
            g[at] ^= delta
            out.append((f"{i}/byte{at}^{delta:02x}", bytes(g), cap))
    for at in bit_stream_tail(f):
        for bit in range(8):
            g = bytearray(f)
            g[at] ^= 1 << bit
            out.append((f"{i}/bits{at}^{1 << bit:02x}", bytes(g), cap))
    for n in range(len(f)):
        out.append((f"{i}/cut{n}", f[:n], cap))
    return out


@functools.lru_cache(None)
def random_damage():
    """300 changes of 1 to 3 bytes, seeds 41000..41299, spread over the bases"""
    bases = damage_bases()
    out = []
    for seed in range(41000, 41300):
        rng = np.random.default_rng(seed)
        i = seed % len(bases)
        f, cap = bases[i]
        g = bytearray(f)
        for _ in range(int(rng.integers(1, 4))):
            g[int(rng.integers(0, len(g)))] = int(rng.integers(0, 256))
        out.append((f"{i}/random{seed}", bytes(g), cap))
    return out
