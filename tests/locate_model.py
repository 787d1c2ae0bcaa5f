"""k_locate_sections (cloudini_amd/csrc/stage1_decode_fast.h) restated in numpy, no GPU: which of its branches locates a
chunk's integer sections, what it leaves in reg_end_pre[c] and in the top byte of slices_done[c], and -- for the decode route
of one adaptive field in front of the point kernel (DC_COLS, stage1_decode_route.h) -- the counters and per-chunk words the
kernels behind it leave. tests/test_locate_model.py holds it to the oracle, tests/test_gpu_locate.py holds the kernels to it.

Everything is written from the kernel's text: the comments name the lines.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NOT_FOUND = 0xFFFFFFFF
K_FAST_PAL_ENTRIES = 1024          # kFastPalEntries


def palette_bits(u: int) -> int:   # stage1_math.h: palette_bits
    return 0 if u <= 1 else (u - 1).bit_length()


def token_ends(payload: np.ndarray) -> np.ndarray:
    """Offsets of the bytes with a clear MSB."""
    return np.nonzero((payload & 0x80) == 0)[0]


def true_section_start(payload: np.ndarray, n: int, n_ops: int):
    """The plain token count: the offset behind token number n * n_ops, None when the payload has fewer."""
    target = n * n_ops
    if target == 0:
        return 0
    ends = token_ends(payload)
    return int(ends[target - 1]) + 1 if len(ends) >= target else None


def _palette_size(u: int, bpv: int, n: int) -> int:
    return 3 + u * bpv + (palette_bits(u) * n + 7) // 8


def pal_guess_from_end(src: np.ndarray, n: int, bpv: int):
    """pal_guess_from_end: four rounds, each the smallest untried U whose header would sit at its place, then the three checks
    of the workgroup. Returns U or None."""
    size = len(src)
    floor = 0
    for _round in range(4):
        cand = None
        for u in range(floor + 1, K_FAST_PAL_ENTRIES + 1):       # (U > floor && S <= src_size), atomicMin
            s = _palette_size(u, bpv, n)
            if s <= size:
                h = size - s
                if src[h] == 1 and (int(src[h + 1]) | (int(src[h + 2]) << 8)) == u:
                    cand = u
                    break
        if cand is None:
            return None
        u = cand
        bits = palette_bits(u)
        off = size - _palette_size(u, bpv, n)
        tab = off + 3
        bad = off != 0 and (src[off - 1] & 0x80) != 0             # tid 0: the token in front would not be over
        if bits != 0:                                             # tid 1..32: index k below U
            idx = tab + u * bpv
            avail = size - idx
            for k in range(min(32, n)):
                bit0 = k * bits
                by = bit0 >> 3
                w = 0
                for b in range(3):
                    if by + b < avail:
                        w |= int(src[idx + by + b]) << (8 * b)
                if ((w >> (bit0 & 7)) & ((1 << bits) - 1)) >= u:
                    bad = True
        entries = [int.from_bytes(bytes(src[tab + i * bpv: tab + (i + 1) * bpv]), "little") for i in range(min(8, u))]
        for i in range(1, len(entries)):                          # tid 33..40: entry i against the entries in front of it
            if entries[i] in entries[:i]:
                bad = True
        if not bad:
            return u
        floor = u
    return None


@dataclass
class Located:
    branch: str            # palette | drle_end | dv_end | front | none
    reg_end_pre: int       # what the kernel writes (NOT_FOUND = 0xffffffff)
    mode_byte: int         # slices_done[c] >> 24
    dv_mode: int           # what the chunk adds to kStatDvMode
    dv_guess: int          # ... and to kStatDvGuess
    right: bool            # a guess: equal to the plain token count's place. front: found at all
    truth: object          # the plain token count's place (None: fewer tokens than the points need)
    dv_candidate: object = None   # the (n + 1)-th end from the back, where the tiles reach it
    drle_candidates: int = 0


def locate(payload, n: int, n_ops: int, bpvs, nw: int, try_dv: int = 1, keep_guess: int = 0, valid: bool = True) -> Located:
    """One workgroup of k_locate_sections<nw> on one chunk."""
    src = np.ascontiguousarray(payload, dtype=np.uint8)
    size = len(src)
    truth = true_section_start(src, n, n_ops)
    none = Located("none", NOT_FOUND, 0xFF, 0, 0, False, truth)
    # :180-182 -- the early returns
    if not valid or len(bpvs) == 0 or len(bpvs) > 8 or any(b > 4 for b in bpvs):
        return none
    ends_mask = (src & 0x80) == 0
    cand_dv = None
    n_cand = 0
    if len(bpvs) == 1:
        bpv = bpvs[0]
        u = pal_guess_from_end(src, n, bpv)                        # :190
        if u is not None:
            off = size - _palette_size(u, bpv, n)
            if keep_guess:                                         # :193-196
                return Located("palette", off, 1, 0, 0, off == truth, truth)
            return Located("palette", NOT_FOUND, 0xFF, 0, 0, off == truth, truth)
        # ---- a lone DeltaRle section from the end, :206-246
        t = nw * 64
        w = t * 16
        wbase = size - w if size > w else 0
        closed = size != 0 and (src[size - 1] & 0x80) == 0         # :221
        cands = []
        if closed:
            win_ends = np.zeros(w + 1, dtype=np.int64)             # ends in window offsets [0, x)
            real = min(w, size - wbase)
            win_ends[1:real + 1] = np.cumsum(ends_mask[wbase:wbase + real])
            win_ends[real + 1:] = win_ends[real]                  # bytes behind the payload read 0xff: no ends
            total = int(win_ends[w])
            for pos in np.nonzero(src[wbase:] == 3)[0] + wbase:
                pos = int(pos)
                x = pos - wbase
                if pos + 5 > size:                                 # :227
                    continue
                if pos != 0 and (src[pos - 1] & 0x80) != 0:        # :228 end_in_front
                    continue
                r = int.from_bytes(bytes(src[pos + 1:pos + 5]), "little")
                if r == 0 or r > n:                                # :231
                    continue
                y = x + 5
                before_y = total if y >= w else int(win_ends[y])   # :233
                if total - before_y != 2 * r:
                    continue
                cands.append(pos)
        n_cand = len(cands)
        if n_cand == 1:                                            # :240-245
            return Located("drle_end", cands[0], 3, 0, 0, cands[0] == truth, truth, None, 1)
        # ---- a lone DeltaVarint section from the end, :252-303
        if closed and n_ops != 0 and try_dv:
            tile = t * 64
            seen, hi = 0, size
            while hi >= tile + 16:                                 # :257
                e = np.nonzero(ends_mask[hi - tile:hi])[0]
                if seen + len(e) >= n + 1:                         # :270 the wanted end lies in this tile
                    want = n + 1 - seen                            # its rank counted from the tile's end, 1-based
                    cand_dv = hi - tile + int(e[len(e) - want])
                    break
                seen += len(e)
                hi -= tile
            if cand_dv is not None and cand_dv >= n * n_ops and src[cand_dv] == 0:   # :294
                return Located("dv_end", cand_dv, 0, 1, 1, cand_dv == truth, truth, cand_dv, n_cand)
    # ---- the count from the front, :305-395
    found = NOT_FOUND if truth is None else truth
    mode = int(src[found]) if found < size else 0xFF
    return Located("front", found, mode, 1 if mode == 0 else 0, 0, truth is not None, truth, cand_dv, n_cand)


def front_part_bytes(size: int, nw: int) -> int:
    """Bytes of the payload each wave of the count from the front takes (:305)."""
    return (((size + 15) // 16 + nw - 1) // nw) * 16


# ---------------------------------------------------------------------------------------------------------------------
# What the route DR_POINTS + DC_COLS leaves behind one chunk whose regular stream the point kernel decodes (valid reference
# streams: no token of more than 5 bytes in the regular stream, the payload ends with its last section), for a FRESH codec
# (no launch hints: k_section_dv_w and k_sections_cols_fast are both launched for one adaptive field).
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class ChunkOutcome:
    sec_cols: int          # 1: a column kernel completed the chunk's columns in front of the point kernel
    dv_chunks: int         # the chunk's share of kStatDvChunks (k_section_dv_w completed it)
    reg_end: int           # reg_end[c] when the call is over
    sec_done: int          # sec_done[c] when the call is over
    words: tuple           # the chunk's share of status words 8..15


def dv_w_completes(src: np.ndarray, off: int, n: int) -> bool:
    """k_section_dv_w (stage1_decode_dv.h) on the bytes behind payload offset `off`: every one of exactly n tokens has 1..5 bytes
    and a value other than 0, the last byte ends a token. (:51-59 the entry conditions, :128 tokens of six bytes and more and
    padded zeros, :181 more tokens than points, :205 a token of value 0, :251 the count.)"""
    sec = src[off + 1:]
    if off >= len(src) or n == 0 or len(sec) < n or (len(sec) and sec[-1] & 0x80):
        return False
    e = np.nonzero((sec & 0x80) == 0)[0]
    if len(e) != n:
        return False
    starts = np.concatenate([[0], e[:-1] + 1])
    lens = e - starts + 1
    if lens.max() > 5:
        return False
    # value 0: every 7-bit group of the token is 0
    low7 = (sec & 0x7F) != 0
    nz = np.add.reduceat(low7.astype(np.int64), starts)
    return bool((nz != 0).all())


def _varint(src, p, size, limit=10):
    """(value of the zigzag + 1 form, next offset) of the varint token at p, None for a token that does not end."""
    v, sh = 0, 0
    for k in range(limit):
        if p + k >= size:
            return None
        b = int(src[p + k])
        v |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            return v, p + k + 1
    return None


def sections_decode_from(payload, off: int, n: int, bpvs) -> bool:
    """decodeV5AdaptiveIntSection for every field from payload offset `off` (the rules of decode_sections_core,
    stage1_decode.h:1702-1878): True when every section decodes and the payload ends with the last one."""
    src = np.ascontiguousarray(payload, dtype=np.uint8)
    size = len(src)
    for bpv in bpvs:
        if off >= size:
            return False
        mode = int(src[off])
        off += 1
        if mode == 0:                                 # n integer tokens; the marker byte is no integer
            for _ in range(n):
                t = _varint(src, off, size)
                if t is None or t[0] == 0:
                    return False
                off = t[1]
        elif mode == 1:
            if size - off < 2:
                return False
            count = int(src[off]) | (int(src[off + 1]) << 8)
            off += 2
            bits = palette_bits(count)
            index_bytes = (bits * n + 7) // 8
            if size - off < count * bpv + index_bytes:
                return False
            off += count * bpv
            if n and count == 0:
                return False
            if bits:
                b = np.unpackbits(src[off:off + index_bytes], bitorder="little")[:bits * n].reshape(n, bits)
                idx = (b.astype(np.int64) << np.arange(bits)).sum(axis=1)
                if (idx >= count).any():
                    return False
            off += index_bytes
        elif mode in (2, 3):
            if size - off < 4:
                return False
            runs = int.from_bytes(bytes(src[off:off + 4]), "little")
            off += 4
            if runs > n:
                return False
            filled = 0
            for _ in range(runs):
                if mode == 2:
                    if size - off < bpv:
                        return False
                    off += bpv
                else:
                    t = _varint(src, off, size)
                    if t is None or t[0] == 0:
                        return False
                    off = t[1]
                t = _varint(src, off, size)
                if t is None or t[0] > n - filled:
                    return False
                filled += t[0]
                off = t[1]
            if filled != n:
                return False
        else:
            return False
    return off == size


def outcome(payload, n: int, n_ops: int, bpvs, loc: Located, sections_ok_from=None) -> ChunkOutcome:
    """The chunk's trace behind the whole call. sections_ok_from(off) -> bool: do the chunk's sections decode from payload offset
    `off` to the payload's end (sections_decode_from above unless the caller has another)."""
    src = np.ascontiguousarray(payload, dtype=np.uint8)
    if sections_ok_from is None:
        sections_ok_from = lambda o: sections_decode_from(src, o, n, bpvs)
    truth = loc.truth
    assert truth is not None, "reference streams hold every point's tokens"
    if loc.branch == "palette":
        # the point kernel makes the guess again (fp_setup, stage1_decode_fast.h:852), folds the table, finds pos == reg_size
        # (stage1_decode_wave.h:733): sec_done 2, words 8, 9 and 12. No column kernel touches the chunk (reg_end_pre is 0xffffffff).
        assert loc.right
        return ChunkOutcome(0, 0, truth, 2, (1, 1, 0, 0, 1, 0, 0, 0))
    off = loc.reg_end_pre
    one = len(bpvs) == 1
    dvc = 1 if (one and loc.mode_byte == 0 and off != NOT_FOUND and dv_w_completes(src, off, n)) else 0
    # k_section_dv_w, else k_sections_cols_fast / k_decode_sections_cols: all of them decode the sections from reg_end_pre and
    # complete the column only if they decode to the payload's end; a column from the RIGHT place is complete whoever made it
    cols = 1 if (dvc or (off != NOT_FOUND and sections_ok_from(off))) else 0
    words = [1, 0, 0, 0, 0, dvc, loc.dv_mode, loc.dv_guess]
    if cols and off == truth:
        # the point kernel merges the columns: pos == reg_size, folded (stage1_decode_wave.h:733-736), sec_done 2
        words[1] = 1
        return ChunkOutcome(1, dvc, truth, 2, tuple(words))
    # No column, or a column from the wrong place (the point kernel stores it, then finds pos != reg_size): not folded, sec_done 0
    # (stage1_decode_wave.h:733-734). k_decode_tail (stage1_decode.h:1925): the chunk's section is no small Palette
    # (decode_sections_small_body leaves at :1666), decode_sections_body decodes it from reg_end[c] -- the place the point pass
    # found -- into the points: sec_done 1 and word 9 (:1905-1908). The serial decoder finds nothing left.
    assert sections_ok_from(truth)
    words[1] = 1
    return ChunkOutcome(cols, dvc, truth, 1, tuple(words))
