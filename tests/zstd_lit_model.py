"""Serial restatement of the device ZSTD writer (cloudini_amd/csrc/zstd_kernels.hip): frames of literal-only blocks.

A frame holds no match: every block is Raw, RLE, or a Compressed block whose literals section is Huffman-coded and whose
sequences section says "0 sequences". Any ZSTD decoder reads such a frame. The kernels are held to byte equality with
frame() below (tests/test_gpu_zstd_encode.py), the frames themselves are judged by libzstd (tests/test_zstd_lit_model.py).

The choices that are this writer's own, and that the kernels restate:
  * a block of fewer than 64 bytes is Raw; a longer one of one byte value is RLE; otherwise it is Compressed unless that
    would not be smaller than the block or its tree description does not fit 127 bytes, then Raw
  * code lengths: the symbols sorted by count << 8 | symbol, Huffman's two queues (a leaf wins a tie against an internal
    node), depths clamped to 11, the number of codes per length repaired to Kraft equality (the longest length below 11 gives
    a code to the next length while the sum is too large; then codes are shortened, the longest first, while one fits the
    deficit), and the lengths handed out over the sorted symbols, the longest to the rarest
  * the tree description: direct for one weight, else FSE with table log 6 and the normalisation of normalise()
The bitstreams come from cumulative sums, not per-symbol loops.
"""
from __future__ import annotations

import numpy as np

BLOCK = 131072
MAX_LEN = 11
MIN_HUF = 64          # a block below this is Raw
FOUR_STREAMS = 256    # four streams from this block size on
RAW, RLE, HUF = 0, 1, 2


def bound(n: int) -> int:
    """libzstd's ZSTD_COMPRESSBOUND"""
    return n + (n >> 8) + (((131072 - n) >> 11) if n < 131072 else 0)


# ---- code lengths ---------------------------------------------------------------------------------------------------------------
def code_lengths(counts: np.ndarray, note=None) -> np.ndarray:
    """counts[256] -> lengths[256] (0 = absent); at least two symbols are present. note["clamped"]: a depth was above 11"""
    keys = sorted((int(c) << 8) | s for s, c in enumerate(counts) if c)
    m = len(keys)
    assert m >= 2
    leaf_w = [k >> 8 for k in keys]
    node_w, node_parent, leaf_parent = [], [0] * (m - 1), [0] * m
    li = ni = 0
    for k in range(m - 1):                                # node k joins the two smallest of what is left
        w = 0
        for _ in range(2):
            take_leaf = li < m and (ni >= len(node_w) or leaf_w[li] <= node_w[ni])
            if take_leaf:
                w += leaf_w[li]
                leaf_parent[li] = k
                li += 1
            else:
                w += node_w[ni]
                node_parent[ni] = k
                ni += 1
        node_w.append(w)
    depth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    per_len = [0] * (MAX_LEN + 1)
    for i in range(m):
        per_len[min(depth[leaf_parent[i]] + 1, MAX_LEN)] += 1
    if note is not None:
        note["clamped"] = any(depth[leaf_parent[i]] + 1 > MAX_LEN for i in range(m))
    full = 1 << MAX_LEN
    kraft = sum(per_len[l] << (MAX_LEN - l) for l in range(1, MAX_LEN + 1))
    while kraft > full:                                   # the longest length below 11 gives a code to the next one
        l = max(x for x in range(1, MAX_LEN) if per_len[x])
        per_len[l] -= 1
        per_len[l + 1] += 1
        kraft -= 1 << (MAX_LEN - 1 - l)
    while kraft < full:                                   # shorten the longest code whose gain fits the deficit
        l = max(x for x in range(2, MAX_LEN + 1) if per_len[x] and (1 << (MAX_LEN - x)) <= full - kraft)
        per_len[l] -= 1
        per_len[l - 1] += 1
        kraft += 1 << (MAX_LEN - l)
    lens = np.zeros(256, np.int64)
    i = 0
    for l in range(MAX_LEN, 0, -1):                        # the longest codes to the rarest symbols
        for _ in range(per_len[l]):
            lens[keys[i] & 255] = l
            i += 1
    assert i == m
    return lens


def code_values(lens: np.ndarray):
    """-> (codes[256], max_len): values go to the longest codes first, from 0; within a length they ascend with the symbol"""
    max_len = int(lens.max())
    per_len = np.bincount(lens, minlength=MAX_LEN + 2)
    first = [0] * (MAX_LEN + 2)
    m = 0
    for l in range(max_len, 0, -1):
        first[l] = m
        m = (m + int(per_len[l])) >> 1
    codes = np.zeros(256, np.int64)
    nxt = list(first)
    for s in range(256):
        l = int(lens[s])
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes, max_len


# ---- tree description -------------------------------------------------------------------------------------------------------------
class Bits:
    """LE bit container"""

    def __init__(self):
        self.v, self.n = 0, 0

    def add(self, value: int, nbits: int):
        self.v |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def bytes(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


def normalise(weights) -> list:
    """counts of the weight values 0 .. max -> normalised counts of sum 64, every value at least 1"""
    top = int(max(weights))
    cnt = np.bincount(np.asarray(weights), minlength=top + 1)
    n = len(weights)
    norm = [max(1, int(c) * 64 // n) for c in cnt]
    big = max(range(top + 1), key=lambda v: (int(cnt[v]), -v))     # the largest count, the smallest value on a tie
    norm[big] += 64 - sum(norm)
    assert norm[big] >= 1
    return norm


def fse_weights(weights) -> bytes:
    """[table description][FSE bitstream of the weights], table log 6, two interleaved states"""
    norm = normalise(weights)
    b = Bits()
    b.add(6 - 5, 4)
    remaining, threshold, nb = 65, 64, 7
    for c in norm:
        mx = 2 * threshold - 1 - remaining
        remaining -= c
        v = c + 1
        if v >= threshold:
            v += mx
        b.add(v, nb - 1 if v < mx else nb)
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    assert remaining == 1
    head = b.bytes()
    # encoding table
    cell = [0] * 64
    pos = 0
    for s, c in enumerate(norm):
        for _ in range(c):
            cell[pos] = s
            pos = (pos + 43) & 63
    assert pos == 0
    cum = [0] * (len(norm) + 1)
    for s, c in enumerate(norm):
        cum[s + 1] = cum[s] + c
    state_table = [0] * 64
    fill = list(cum)
    for u in range(64):
        state_table[fill[cell[u]]] = 64 + u
        fill[cell[u]] += 1
    delta_nb, delta_state = [], []
    total = 0
    for c in norm:
        if c == 1:
            delta_nb.append((6 << 16) - 64)
            delta_state.append(total - 1)
        else:
            out = 6 - ((c - 1).bit_length() - 1)
            delta_nb.append((out << 16) - (c << out))
            delta_state.append(total - c)
        total += c
    b = Bits()
    state = [None, None]                                  # state 1 (even indexes), state 2 (odd indexes)
    for i in range(len(weights) - 1, -1, -1):
        w = int(weights[i])
        k = i & 1
        if state[k] is None:
            nbo = (delta_nb[w] + 32768) >> 16
            v = (nbo << 16) - delta_nb[w]
            state[k] = state_table[(v >> nbo) + delta_state[w]]
        else:
            nbo = (state[k] + delta_nb[w]) >> 16
            b.add(state[k], nbo)
            state[k] = state_table[(state[k] >> nbo) + delta_state[w]]
    b.add(state[1], 6)
    b.add(state[0], 6)
    b.add(1, 1)
    return head + b.bytes()


def tree_description(lens: np.ndarray, max_len: int):
    """-> bytes, or None when the description does not fit"""
    last = int(np.nonzero(lens)[0][-1])
    weights = [int(max_len + 1 - l) if l else 0 for l in lens[:last]]
    if len(weights) == 1:
        return bytes([127 + 1, weights[0] << 4])
    body = fse_weights(weights)
    if len(body) >= 128:
        return None
    return bytes([len(body)]) + body


# ---- blocks -----------------------------------------------------------------------------------------------------------------------
def stream_bytes(sym: np.ndarray, lens: np.ndarray, codes: np.ndarray) -> bytes:
    """the stream's last symbol at bit 0, the first at the top, then a 1 bit, zeros to the byte"""
    l = lens[sym][::-1]
    c = codes[sym][::-1]
    pos = np.cumsum(l) - l
    total = int(l.sum())
    bits = np.zeros((total // 8 + 1) * 8, np.uint8)
    for k in range(MAX_LEN):
        sel = l > k
        bits[pos[sel] + k] = (c[sel] >> k) & 1
    bits[total] = 1
    return np.packbits(bits, bitorder="little").tobytes()


def literals_header(regen: int, comp: int, four: bool):
    """-> (form, bytes)"""
    if not four:
        assert regen < 1024 and comp < 1024
        form, bits, size = 0, 10, 3
    elif regen < 1024 and comp < 1024:
        form, bits, size = 1, 10, 3
    elif regen < 16384 and comp < 16384:
        form, bits, size = 2, 14, 4
    else:
        assert regen < 262144 and comp < 262144
        form, bits, size = 3, 18, 5
    v = 2 | (form << 2) | (regen << 4) | (comp << (4 + bits))
    return form, v.to_bytes(size, "little")


def block_header(last: bool, kind: int, size: int) -> bytes:
    return (int(last) | (kind << 1) | (size << 3)).to_bytes(3, "little")


def block(data: np.ndarray, last: bool, note=None):
    """-> (kind, header form or None, bytes). note (a dict) takes what the block went through: why it is Raw, the number of
    weights and the form of the tree description, whether lengths were clamped, the stream sizes"""
    note = {} if note is None else note
    n = data.size
    note.update(n=n, kind=RAW, form=None)
    raw = (RAW, None, block_header(last, RAW, n) + data.tobytes())
    if n < MIN_HUF:
        note["why_raw"] = "short"
        return raw
    counts = np.bincount(data, minlength=256)
    if np.count_nonzero(counts) == 1:
        note["kind"] = RLE
        return RLE, None, block_header(last, RLE, n) + data[:1].tobytes()
    lens = code_lengths(counts, note)
    codes, max_len = code_values(lens)
    desc = tree_description(lens, max_len)
    note.update(symbols=int(np.count_nonzero(counts)), weights=int(np.nonzero(lens)[0][-1]), max_len=max_len,
                description=None if desc is None else "direct" if desc[0] >= 128 else "fse")
    if desc is None:
        note["why_raw"] = "description"
        return raw
    four = n >= FOUR_STREAMS
    if four:
        seg = (n + 3) // 4
        streams = [stream_bytes(data[k * seg:min(n, (k + 1) * seg)], lens, codes) for k in range(4)]
        jump = b"".join(len(s).to_bytes(2, "little") for s in streams[:3])
    else:
        streams, jump = [stream_bytes(data, lens, codes)], b""
    comp = len(desc) + len(jump) + sum(len(s) for s in streams)
    note["streams"] = [len(s) for s in streams]
    if comp >= 262144:
        return raw
    hdr_size = 3 if (not four or (n < 1024 and comp < 1024)) else 4 if (n < 16384 and comp < 16384) else 5
    if hdr_size + comp + 1 >= n:
        note["why_raw"] = "not smaller"
        return raw
    form, hdr = literals_header(n, comp, four)
    note.update(kind=HUF, form=form, comp=comp)
    body = hdr + desc + jump + b"".join(streams) + b"\x00"
    return HUF, form, block_header(last, HUF, len(body)) + body


def frame_info(payload, trace=None):
    """-> (frame bytes, [(kind, header form)] per block); trace (a list) takes block()'s note of every block"""
    data = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8).ravel()
    n = data.size
    out = [b"\x28\xb5\x2f\xfd\xa0", n.to_bytes(4, "little")]
    kinds = []
    if n == 0:
        out.append(block_header(True, RAW, 0))
        kinds.append((RAW, None))
        if trace is not None:
            trace.append(dict(n=0, kind=RAW, form=None, why_raw="short"))
    for o in range(0, n, BLOCK):
        note = {}
        if trace is not None:
            trace.append(note)
        kind, form, b = block(data[o:o + BLOCK], o + BLOCK >= n, note)
        out.append(b)
        kinds.append((kind, form))
    return b"".join(out), kinds


def frame(payload) -> bytes:
    return frame_info(payload)[0]
