"""The rules of the device ZSTD decoder with the sequences switch on (cloudini_amd/csrc/zstd_decode_walk.h zd_walk_seq,
zstd_seq_decode.hip), restated serially. A superset of tests/zstd_lit_rules.py: every frame that module calls OK or CORRUPT
keeps its verdict and bytes; a frame it calls HOST only because a block has nbSeq != 0 is judged here. No GPU.

decode(frame, capacity) -> (verdict, payload)          the three verdicts of zstd_lit_rules
decode_trace(frame, capacity) -> (verdict, payload, trace)

Order of judgement, as on the device: the walk (headers, table descriptions: the first finding in frame order), and only if
that is OK: the literal streams and the sequence bit streams of all blocks (the worst finding), then the execution (its
first finding: it is serial and its state depends on what came before).

What is HOST here beyond zstd_lit_rules, and why (libzstd's versions are not one rule set; 1.4.8 is the one pinned):
  * Reserved bits of the modes byte not zero: 1.4.8 ignores them, 1.5 refuses them.
  * nbSeq == 0 written in the 2- or 3-byte form: 1.4.8 reads the tables and executes nothing; later versions differ.
  * A repeat offset `rep1 - 1` that gives 0: 1.4.8 forces it to 1, 1.5 calls it corruption. The execution stops there.
  * The bit stream is not consumed exactly when the last sequence has been read. Bits left: 1.4.8 refuses, versions up to
    1.4.5 do not look. A stream that ran over its start, at any sequence (zeros are read there): up to 1.4.5 the loop
    stops and the frame is refused, 1.4.8 reloads without looking and accepts. (The issue expected CORRUPT for the second;
    the pinned 1.4.8 accepts such frames, so no stream-end finding is CORRUPT.)
  * An offset code of 30 or 31: the device packs the offset value into 30 bits.
  * A block that regenerates more than the frame's block maximum: 1.4.8 only holds it against the room that is left, later
    versions refuse. (More than `capacity` in total is CORRUPT in all.)
  * A window above 16 MiB in a frame with sequences: libzstd may choose its long-offset decoder, whose end-of-stream checks
    differ.
  * Blocks: a frame with a sequence block lists EVERY block (the empty ones too) against a record limit of its own,
    4 + bytes / 16 + capacity / 128 KiB.
CORRUPT beyond zstd_lit_rules: an RLE symbol above 35 / 31 / 52; a table description that does not parse within the block,
with an accuracy log above 9 / 8 / 9 or symbols beyond the alphabet; Repeat mode with no earlier sequence block in the frame;
no bit stream, or its last byte 0; literals that run out; an offset beyond the bytes produced so far (there is no
dictionary); sum(nbSeq) above capacity / 3 (a match has at least 3 bytes) or literals above `capacity`; a total beyond
`capacity` or different from the content size.
"""
from __future__ import annotations

import zstd_lit_rules as R
from zstd_lit_rules import BLOCK_MAX, CORRUPT, HOST, HUF, NO_TREE, OK, RAW, RLE, worst

PREDEFINED, MODE_RLE, FSE, REPEAT = 0, 1, 2, 3
LL, OF, ML = 0, 1, 2
MAX_SYM = (35, 31, 52)
MAX_LOG = (9, 8, 9)
DEFAULT_LOG = (6, 5, 6)
DEFAULT_NORM = (
    [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1],
    [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1],
    [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7,
)
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
MAX_OF_CODE = 29
LONG_WINDOW = 1 << 24
NO_REC = 0xFFFFFFFF


def read_norm(buf: bytes, max_log: int, max_sym: int):
    """the normalised counts at the start of buf -> (verdict, counts, accuracy log, bytes used)"""
    n = len(buf)
    word = int.from_bytes(buf, "little")
    log = (word & 15) + 5
    at = 4
    if log > max_log:
        return CORRUPT, None, 0, 0
    size = 1 << log
    remaining, threshold, nb = size + 1, size, log + 1
    norm = []
    prev0 = False
    while remaining > 1 and len(norm) <= max_sym:
        if prev0:
            n0 = len(norm)
            while True:
                r = (word >> at) & 3
                at += 2
                n0 += r
                if n0 > max_sym or at > 8 * n:
                    return CORRUPT, None, 0, 0
                if r != 3:
                    break
            norm.extend([0] * (n0 - len(norm)))
        mx = 2 * threshold - 1 - remaining
        low = (word >> at) & (threshold - 1)
        if low < mx:
            c = low
            at += nb - 1
        else:
            c = (word >> at) & (2 * threshold - 1)
            if c >= threshold:
                c -= mx
            at += nb
        c -= 1
        remaining -= abs(c)
        norm.append(c)
        prev0 = c == 0
        while remaining < threshold and threshold > 1:
            nb -= 1
            threshold >>= 1
    if remaining != 1 or at > 8 * n:
        return CORRUPT, None, 0, 0
    return OK, norm, log, (at + 7) // 8


def fse_table(norm, log):
    """-> [(symbol, bits, baseline)] * 2^log"""
    size = 1 << log
    sym = [0] * size
    nxt = []
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt.append(1)
        else:
            nxt.append(c)
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    table = []
    for u in range(size):
        x = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb = log - (x.bit_length() - 1)
        table.append((sym[u], nb, (x << nb) - size))
    return table


def read_seq_header(f: bytes, q: int, end: int):
    """the sequences section f[q:end] with nbSeq != 0 -> (verdict, dict(nb, form, modes, tab [(at, bytes)], norm, bits (a, b)))"""
    b0 = f[q]
    if b0 < 128:
        nb, form = b0, 1
    elif b0 < 255:
        if q + 2 > end:
            return CORRUPT, None
        nb, form = ((b0 - 128) << 8) + f[q + 1], 2
    else:
        if q + 3 > end:
            return CORRUPT, None
        nb, form = f[q + 1] + (f[q + 2] << 8) + 0x7F00, 3
    p = q + form
    if p + 1 > end:
        return CORRUPT, None
    mb = f[p]
    p += 1
    if nb == 0 or mb & 3:
        return HOST, None
    modes = [(mb >> 6) & 3, (mb >> 4) & 3, (mb >> 2) & 3]
    tab, norms = [], []
    for t in range(3):
        m = modes[t]
        if m == MODE_RLE:
            if p >= end or f[p] > MAX_SYM[t]:
                return CORRUPT, None
            tab.append((p, 1))
            norms.append(None)
            p += 1
        elif m == FSE:
            v, norm, log, used = read_norm(f[p:end], MAX_LOG[t], MAX_SYM[t])
            if v != OK:
                return v, None
            tab.append((p, used))
            norms.append((norm, log))
            p += used
        else:
            tab.append((0, 0))
            norms.append(None)
    if p >= end or f[end - 1] == 0:
        return CORRUPT, None
    return OK, dict(nb=nb, form=form, modes=modes, tab=tab, norm=norms, bits=(p, end))


def walk(frame: bytes, capacity: int, all_blocks: bool = None, max_blocks: int = 1 << 30, read_trees: bool = True, note: dict = None):
    """-> (verdict, blocks, sums). all_blocks=None: the counting pass decides it (as decode() does).
    A frame without a sequence block: zstd_lit_rules' records. With one: EVERY block is listed, `out` is the place of its
    literals in the frame's literal buffer, `order` its number, and block["seq"] is None or read_seq_header's dict plus
    rep [record whose table a Repeat mode means, per table] and first (its first sequence among the frame's).
    sums: dict(seqs, lits, has_seq, n_all, n_regen, total (of a frame without sequences), fcs, block_max)."""
    f = bytes(frame)
    n = len(f)
    blocks = []
    sums = dict(seqs=0, lits=0, has_seq=False, n_all=0, n_regen=0, total=0, fcs=None, block_max=0)

    def seen(a, b):
        if note is not None:
            note.setdefault("seq_headers", []).append((a, b))
    if n == 0:
        return HOST, blocks, sums
    if n < 5:
        return CORRUPT, blocks, sums
    magic = int.from_bytes(f[:4], "little")
    if magic & 0xFFFFFFF0 == 0x184D2A50:
        return HOST, blocks, sums
    if magic != 0xFD2FB528:
        return CORRUPT, blocks, sums
    fhd = f[4]
    if fhd & 8:
        return CORRUPT, blocks, sums
    if fhd & 7:
        return HOST, blocks, sums
    single = (fhd >> 5) & 1
    fcs_bytes = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    p = 5
    if n < p + (0 if single else 1) + fcs_bytes:
        return CORRUPT, blocks, sums
    window = None
    if not single:
        wd = f[p]
        p += 1
        wlog = 10 + (wd >> 3)
        if wlog > 27:
            return HOST, blocks, sums
        window = (1 << wlog) + ((1 << wlog) >> 3) * (wd & 7)
    fcs = None
    if fcs_bytes:
        fcs = int.from_bytes(f[p:p + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0)
        p += fcs_bytes
    if single:
        window = fcs
    block_max = min(window, BLOCK_MAX)
    sums["fcs"], sums["block_max"] = fcs, block_max
    total = 0
    tree = NO_TREE
    last_def = [NO_REC] * 3
    seq_before = False
    while True:
        if n - p < 3:
            return CORRUPT, blocks, sums
        bh = int.from_bytes(f[p:p + 3], "little")
        p += 3
        last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
        if kind == 3:
            return CORRUPT, blocks, sums
        rec = None
        seq = None
        if kind == RAW:
            if size > n - p:
                return CORRUPT, blocks, sums
            if size > block_max:
                return HOST, blocks, sums
            rec = dict(kind=RAW, src=p, size=size, regen=size, streams=0, tree=NO_TREE, desc=0)
            p += size
        elif kind == RLE:
            if n - p < 1:
                return CORRUPT, blocks, sums
            if size > block_max:
                return HOST, blocks, sums
            rec = dict(kind=RLE, src=p, size=1, regen=size, streams=0, tree=NO_TREE, desc=0)
            p += 1
        else:
            if size > n - p or size >= BLOCK_MAX or size < 3:
                return CORRUPT, blocks, sums
            if size > block_max:
                return HOST, blocks, sums
            end = p + size
            b0 = f[p]
            lt, sf = b0 & 3, (b0 >> 2) & 3
            if lt < 2:
                lh = (1, 2, 1, 3)[sf]
                if lt == 1 and lh == 3 and size < 4:
                    return CORRUPT, blocks, sums
                regen = int.from_bytes(f[p:p + lh], "little") >> (3 if lh == 1 else 4)
                if regen > BLOCK_MAX:
                    return CORRUPT, blocks, sums
                body = regen if lt == 0 else 1
                if lh + body > size:
                    return CORRUPT, blocks, sums
                rec = dict(kind=RAW if lt == 0 else RLE, src=p + lh, size=body, regen=regen, streams=0, tree=NO_TREE, desc=0)
                q = p + lh + body
            else:
                if size < 5:
                    return CORRUPT, blocks, sums
                lh = (3, 3, 4, 5)[sf]
                v = int.from_bytes(f[p:p + 5], "little")
                nbits = (10, 10, 14, 18)[sf]
                regen = (v >> 4) & ((1 << nbits) - 1)
                comp = (v >> (4 + nbits)) & ((1 << nbits) - 1)
                streams = 1 if sf == 0 else 4
                if regen > BLOCK_MAX:
                    return CORRUPT, blocks, sums
                if lh + comp > size:
                    return CORRUPT, blocks, sums
                if lt == 3 and tree == NO_TREE:
                    return CORRUPT, blocks, sums
                if regen == 0:
                    return HOST, blocks, sums
                if comp == 0:
                    return CORRUPT, blocks, sums
                if streams == 4 and regen - 3 * ((regen + 3) // 4) < 1:
                    return HOST, blocks, sums
                rec = dict(kind=HUF, src=p + lh, size=comp, regen=regen, streams=streams, tree=tree, desc=0)
                if lt == 2 and not read_trees:
                    tree = rec["tree"] = len(blocks)
                elif lt == 2:
                    wv, w, log, used = R.read_weights(f[p + lh:p + lh + comp])
                    if wv != OK:
                        return wv, blocks, sums
                    if used >= comp:
                        return CORRUPT, blocks, sums
                    rec.update(desc=used, log=log, weights=w, tree=len(blocks))
                    tree = len(blocks)
                if read_trees and streams == 4 and comp - rec["desc"] < 10:
                    return CORRUPT, blocks, sums
                q = p + lh + comp
            if regen > block_max:
                return HOST, blocks, sums
            if q >= end:
                return CORRUPT, blocks, sums
            if f[q] != 0:
                sums["has_seq"] = True
                if all_blocks is False:              # (the counting pass said otherwise: it cannot happen)
                    return HOST, blocks, sums
                if read_trees:
                    if window > LONG_WINDOW:
                        return HOST, blocks, sums
                    sv, seq = read_seq_header(f, q, end)
                    if sv != OK:
                        return sv, blocks, sums
                    for t in range(3):
                        seen(*((seq["tab"][t][0], sum(seq["tab"][t])) if seq["tab"][t][1] else (q, q)))
                    seen(q, q + seq["form"] + 1)
                    seq["rep"] = [NO_REC] * 3
                    for t in range(3):
                        if seq["modes"][t] == REPEAT:
                            if not seq_before:
                                return CORRUPT, blocks, sums
                            seq["rep"][t] = last_def[t]
                        else:
                            last_def[t] = len(blocks)
                    seq_before = True
                    seq["first"] = sums["seqs"]
                    sums["seqs"] += seq["nb"]
                    if 3 * sums["seqs"] > capacity:
                        return CORRUPT, blocks, sums
            elif q + 1 != end:
                return CORRUPT, blocks, sums
            p = end
        if sums["lits"] + rec["regen"] > capacity:
            return CORRUPT, blocks, sums
        if not sums["has_seq"] and total + rec["regen"] > capacity:
            return CORRUPT, blocks, sums
        rec["out"] = sums["lits"] if all_blocks else total
        rec["order"] = sums["n_all"]
        rec["seq"] = seq
        total += rec["regen"]
        sums["lits"] += rec["regen"]
        sums["total"] = total
        sums["n_all"] += 1
        sums["n_regen"] += 1 if rec["regen"] else 0
        if rec["regen"] or all_blocks:
            if len(blocks) >= max_blocks:
                return HOST, blocks, sums
            blocks.append(rec)
        if last:
            break
    if not sums["has_seq"] and fcs is not None and fcs != total:
        return CORRUPT, blocks, sums
    if p != n:
        return HOST, blocks, sums
    return OK, blocks, sums


def _table_of(f, blocks, i, t):
    """the decode table of table t of block i"""
    seq = blocks[i]["seq"]
    m = seq["modes"][t]
    if m == REPEAT:
        return _table_of(f, blocks, seq["rep"][t], t)
    if m == PREDEFINED:
        return fse_table(DEFAULT_NORM[t], DEFAULT_LOG[t]), DEFAULT_LOG[t]
    if m == MODE_RLE:
        return [(f[seq["tab"][t][0]], 0, 0)], 0
    norm, log = seq["norm"][t]
    return fse_table(norm, log), log


def decode_sequences(f: bytes, blocks, i):
    """the bit stream of block i -> (verdict, [(ll, ml, offset value)])"""
    seq = blocks[i]["seq"]
    tabs = [_table_of(f, blocks, i, t) for t in range(3)]
    a, b = seq["bits"]
    s = f[a:b]
    word = int.from_bytes(s, "little")
    pos = 8 * (len(s) - 1) + s[-1].bit_length() - 1

    def back(k):
        nonlocal pos
        pos -= k
        if pos >= 0:
            return (word >> pos) & ((1 << k) - 1)
        return ((word << -pos) & ((1 << k) - 1)) if -pos < k else 0
    st = [back(tabs[t][1]) for t in (LL, OF, ML)]
    out = []
    verdict = OK
    for k in range(seq["nb"]):
        if pos < 0:
            return HOST, out
        ll_s, of_s, ml_s = (tabs[t][0][st[t]] for t in (LL, OF, ML))
        if of_s[0] > MAX_OF_CODE:
            verdict = worst(verdict, HOST)
        ofv = (1 << of_s[0]) + back(of_s[0])
        ml = ML_BASE[ml_s[0]] + back(ML_BITS[ml_s[0]])
        ll = LL_BASE[ll_s[0]] + back(LL_BITS[ll_s[0]])
        out.append((ll, ml, ofv))
        if k + 1 < seq["nb"]:
            st[LL] = ll_s[2] + back(ll_s[1])
            st[ML] = ml_s[2] + back(ml_s[1])
            st[OF] = of_s[2] + back(of_s[1])
    if pos != 0:
        verdict = worst(verdict, HOST)
    return verdict, out


def decode_literals(f: bytes, blocks, blk):
    """-> (verdict, the block's literals)"""
    src, regen = blk["src"], blk["regen"]
    if blk["kind"] == RAW:
        return OK, f[src:src + regen]
    if blk["kind"] == RLE:
        return OK, f[src:src + 1] * regen
    t = blocks[blk["tree"]]
    table = R.build_table(t["weights"], t["log"])
    data = f[src + blk["desc"]:src + blk["size"]]
    if blk["streams"] == 1:
        spans = [(0, len(data), regen)]
    else:
        l = [int.from_bytes(data[2 * k:2 * k + 2], "little") for k in range(3)]
        if 6 + sum(l) > len(data):
            return CORRUPT, b""
        seg = (regen + 3) // 4
        l.append(len(data) - 6 - sum(l))
        spans, at = [], 6
        for k in range(4):
            spans.append((at, l[k], seg if k < 3 else regen - 3 * seg))
            at += l[k]
    verdict = OK
    out = bytearray(regen)
    at = 0
    for so, sn, cnt in spans:
        v, sym = R.decode_stream(data[so:so + sn], cnt, table, t["log"])
        verdict = worst(verdict, v)
        out[at:at + len(sym)] = sym
        at += cnt
    return verdict, bytes(out)


def record_limit(n, capacity, has_seq=False):
    """block records the device gives a frame: zstd_lit_rules' for a frame without sequences; one with sequences lists every
    block, and a block with sequences may be as small as 7 bytes"""
    return 4 + n // 16 + capacity // BLOCK_MAX if has_seq else R.record_limit(n, capacity)


def decode_trace(frame: bytes, capacity: int):
    f = bytes(frame)
    trace = dict(blocks=[], rep=set(), max_offset=0, overlap=False, cross_block=False, has_seq=False)
    cv, cblocks, csums = walk(f, capacity, all_blocks=None, read_trees=False)
    all_blocks = csums["has_seq"]
    counted = (csums["n_all"] if all_blocks else csums["n_regen"]) + (cv != OK)
    if counted > record_limit(len(f), capacity, all_blocks):
        return HOST, None, trace
    verdict, blocks, sums = walk(f, capacity, all_blocks=all_blocks)
    if verdict != OK:
        return verdict, None, trace
    trace["has_seq"] = all_blocks
    lits, seqs = [], []
    for i, blk in enumerate(blocks):
        v, l = decode_literals(f, blocks, blk)
        verdict = worst(verdict, v)
        lits.append(l)
        s = None
        if blk["seq"] is not None:
            v, s = decode_sequences(f, blocks, i)
            verdict = worst(verdict, v)
            trace["blocks"].append(dict(modes=tuple(blk["seq"]["modes"]), nb=blk["seq"]["nb"], form=blk["seq"]["form"]))
        seqs.append(s)
    if verdict != OK:
        return verdict, None, trace
    out = bytearray()
    rep = [1, 4, 8]
    for i, blk in enumerate(blocks):
        start = len(out)
        l = lits[i]
        lp = 0
        for ll, ml, ofv in seqs[i] or []:
            if ll > len(l) - lp:
                return CORRUPT, None, trace
            out += l[lp:lp + ll]
            lp += ll
            if ofv > 3:
                off = ofv - 3
                rep = [off, rep[0], rep[1]]
            else:
                idx = ofv - 1 + (1 if ll == 0 else 0)
                trace["rep"].add((ofv, ll == 0))
                if idx == 0:
                    off = rep[0]
                elif idx == 1:
                    off = rep[1]
                    rep = [rep[1], rep[0], rep[2]]
                elif idx == 2:
                    off = rep[2]
                    rep = [rep[2], rep[0], rep[1]]
                else:
                    off = rep[0] - 1
                    if off == 0:
                        return HOST, None, trace
                    rep = [off, rep[0], rep[1]]
            if off > len(out):
                return CORRUPT, None, trace
            if len(out) + ml > capacity:
                return CORRUPT, None, trace
            trace["max_offset"] = max(trace["max_offset"], off)
            trace["overlap"] |= off < ml
            trace["cross_block"] |= len(out) - off < start
            at = len(out) - off
            if off >= ml:
                out += out[at:at + ml]
            else:
                for k in range(ml):
                    out.append(out[at + k])
        out += l[lp:]
        if len(out) > capacity:
            return CORRUPT, None, trace
        if len(out) - start > sums["block_max"]:
            return HOST, None, trace
    if sums["fcs"] is not None and sums["fcs"] != len(out):
        return CORRUPT, None, trace
    return OK, bytes(out), trace


def decode(frame: bytes, capacity: int):
    v, payload, _ = decode_trace(frame, capacity)
    return v, payload
