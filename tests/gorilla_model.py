"""Plain-Python restatement of the Gorilla codec for doubles (FieldEncoderFloat_Gorilla<double> / FieldDecoderFloat_Gorilla<double>,
include/cloudini_lib/field_encoder.hpp:156-312, field_decoder.hpp:158-305, read through oracle/cloudini_oracle.c OP_GORILLA64) and of
what the device decoder does with such a stream (k_decode_stream_w<12, 2>, cloudini_amd/csrc/stage1_decode_stream.h). Pure CPU, no
library of the project is loaded. Four parts:

  encoder / decoder   encode_trace, encode_tokens, decode_tokens
  inverse builder     values_for(specs): the bit patterns from which the encoder writes exactly the wanted tokens
  raw token writer    tok_first / tok_repeat / tok_reuse / tok_open: any token a decoder accepts, also those no encoder writes
  fallback model      parse_regular, serial_expected: the pieces of a chunk, the points and rounds of each, and whether the
                      parallel decoder hands the chunk to the serial one

A token: bits LSB-first, flushed to a whole byte (the padding bits are zero from the encoder and ignored by the decoders).
  first value of a chunk   64 raw bits
  '0'                      the value before, again                                   1 byte
  '1','0' + m bits         (x >> T) under the window (L, T) in effect, m = 64 - L - T
  '1','1' + 5 + 6 + m      stored leading = min(clz, 31), m - 1, (x >> ctz); m = 64 - stored - ctz; the window becomes (stored, ctz)
A window is None (kLeadingSentinel) or (leading, trailing).
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
PIECE = 1024            # kSwPiece: bytes of a decoder piece, at 16-byte aligned addresses
MAX_ROUNDS = 40         # kSwMaxRounds
MAX_POINT_BYTES = 88    # kSwMaxPointBytes
LEAD_VARINT_SPAN = 64   # make_jt_gor: the varints a point begins with must end within 64 bytes of the point's 16-byte unit
CHUNK = 32768


class GorillaError(ValueError):
    """What the reference's decoder throws on (and the oracle returns an error for): kind = 'corrupt' | 'truncated'."""

    def __init__(self, kind, what):
        super().__init__("%s: %s" % (kind, what))
        self.kind = kind


def clz64(x):
    return 64 - int(x).bit_length()


def ctz64(x):
    x = int(x)
    return (x & -x).bit_length() - 1


# ---------------------------------------------------------------------------------------------------------------------
# raw token writer
# ---------------------------------------------------------------------------------------------------------------------
def _flush(parts, pad=0):
    """[(value, bits)] LSB-first -> bytes; `pad` fills the unused high bits of the last byte."""
    acc = n = 0
    for v, nb in parts:
        acc |= (int(v) & ((1 << nb) - 1)) << n
        n += nb
    size = (n + 7) // 8
    free = 8 * size - n
    acc |= (int(pad) & ((1 << free) - 1)) << n
    return acc.to_bytes(size, "little")


def tok_first(value):
    return int(value).to_bytes(8, "little")


def tok_repeat(pad=0):
    return _flush([(0, 1)], pad)


def tok_reuse(window, payload, pad=0):
    lead, trail = window
    return _flush([(1, 2), (payload, 64 - lead - trail)], pad)


def tok_open(stored_leading, m, payload, pad=0):
    """Any '11' token: stored_leading 0..31, m 1..64 -- also stored_leading + m > 64, which every decoder here refuses."""
    return _flush([(3, 2), (stored_leading, 5), (m - 1, 6), (payload, m)], pad)


# ---------------------------------------------------------------------------------------------------------------------
# encoder / decoder
# ---------------------------------------------------------------------------------------------------------------------
def encode_trace(bits):
    """-> (tokens, kinds, windows): per value the token's bytes, 'first' | '0' | '10' | '11', and the window BEHIND it."""
    tokens, kinds, windows = [], [], []
    prev, win = 0, None
    for i, cur in enumerate(int(b) for b in bits):
        if i == 0:
            tokens.append(tok_first(cur))
            kinds.append("first")
        else:
            x = cur ^ prev
            if x == 0:
                tokens.append(tok_repeat())
                kinds.append("0")
            else:
                lead, trail = clz64(x), ctz64(x)
                if win is not None and lead >= win[0] and trail >= win[1]:
                    tokens.append(tok_reuse(win, x >> win[1]))
                    kinds.append("10")
                else:
                    stored = min(lead, 31)
                    tokens.append(tok_open(stored, 64 - stored - trail, x >> trail))
                    kinds.append("11")
                    win = (stored, trail)
        prev = cur
        windows.append(win)
    return tokens, kinds, windows


def encode_tokens(bits):
    return encode_trace(bits)[0]


def read_token(buf, pos, first, win):
    """The token at buf[pos:]: -> (length, xor difference or the raw first value, kind, window behind it)."""
    def need(k):
        if pos + k > len(buf):
            raise GorillaError("truncated", "token at byte %d needs %d bytes, %d left" % (pos, k, len(buf) - pos))
        return int.from_bytes(bytes(buf[pos:pos + k]), "little")
    if first:
        return 8, need(8), "first", win
    b0 = need(1)
    if (b0 & 1) == 0:
        return 1, 0, "0", win
    if (b0 & 2) == 0:
        if win is None or win[0] + win[1] >= 64:
            raise GorillaError("corrupt", "'10' token without a window at byte %d" % pos)
        m = 64 - win[0] - win[1]
        size = (2 + m + 7) // 8
        return size, ((need(size) >> 2) & ((1 << m) - 1)) << win[1], "10", win
    hdr = need(2)
    stored, m = (hdr >> 2) & 31, ((hdr >> 7) & 63) + 1
    size = (13 + m + 7) // 8
    w = need(size)
    if stored + m > 64:
        raise GorillaError("corrupt", "'11' token with leading %d + meaningful %d > 64 at byte %d" % (stored, m, pos))
    trail = 64 - stored - m
    return size, ((w >> 13) & ((1 << m) - 1)) << trail, "11", (stored, trail)


def decode_tokens(tokens):
    """The values of a list of tokens (or of their bytes in one buffer): uint64[n]."""
    buf = b"".join(tokens) if isinstance(tokens, (list, tuple)) else bytes(tokens)
    out, pos, prev, win = [], 0, 0, None
    while pos < len(buf):
        size, x, kind, win = read_token(buf, pos, not out, win)
        prev = x if kind == "first" else prev ^ x
        out.append(prev)
        pos += size
    return np.array(out, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# inverse builder
# ---------------------------------------------------------------------------------------------------------------------
def default_payload(width):
    """`width` meaningful bits with the highest and the lowest set (so clz and ctz are exactly what the caller chose)."""
    return (1 << (width - 1)) | 1


def values_for(specs, first=0x3FF0000000000000):
    """Bit patterns from which the reference's encoder writes exactly the tokens of `specs`, behind the raw `first` value.
    A specification: ('0',) | ('10', payload) | ('11', clz, ctz, payload); payload None = default_payload of the width.
    '10': payload = x >> T under the window in effect (64 - L - T bits, not 0). '11': payload = x >> ctz, 64 - clz - ctz bits wide with
    the highest and lowest bit set. Raises ValueError for what the encoder would not write: a '10' without a window or beyond it,
    a '11' whose difference fits the window in effect (the encoder reuses the window then)."""
    out, prev, win = [int(first)], int(first), None
    for k, s in enumerate(specs):
        if s[0] == "0":
            x = 0
        elif s[0] == "10":
            if win is None:
                raise ValueError("spec %d: '10' without a window" % k)
            m = 64 - win[0] - win[1]
            pay = default_payload(m) if s[1] is None else int(s[1])
            if pay <= 0 or pay >> m:
                raise ValueError("spec %d: '10' payload %#x is 0 or wider than the window's %d bits" % (k, pay, m))
            x = pay << win[1]
        elif s[0] == "11":
            lead, trail = int(s[1]), int(s[2])
            width = 64 - lead - trail
            if not (0 <= lead <= 63 and 0 <= trail <= 63 and width >= 1):
                raise ValueError("spec %d: no difference has clz %d and ctz %d" % (k, lead, trail))
            pay = default_payload(width) if s[3] is None else int(s[3])
            if pay.bit_length() != width or (pay & 1) == 0:
                raise ValueError("spec %d: '11' payload %#x does not have clz %d / ctz %d" % (k, pay, lead, trail))
            if win is not None and lead >= win[0] and trail >= win[1]:
                raise ValueError("spec %d: clz %d / ctz %d fits the window %r: the encoder writes '10'" % (k, lead, trail, win))
            x = pay << trail
            win = (min(lead, 31), trail)
        else:
            raise ValueError("spec %d: %r" % (k, s))
        prev ^= x
        out.append(prev)
    return np.array(out, dtype=np.uint64)


def windows_in_front(bits, piece_pts):
    """What k_gorilla_windows must publish for a chunk: the window in effect in front of the first point of every encoder piece
    of `piece_pts` points (504 with 3 float lanes, 378 with 4)."""
    _t, _k, wins = encode_trace(bits)
    return [None if p == 0 else wins[p - 1] for p in range(0, len(wins), piece_pts)]


# ---------------------------------------------------------------------------------------------------------------------
# the regular stream of a chunk: ops are 'v' (a varint token), ('r', size) (raw bytes) and 'g' (a Gorilla token)
# ---------------------------------------------------------------------------------------------------------------------
def varint(d):
    """encodeVarint64 (encoding_utils.hpp): zig-zag + 1 (0 is the NaN marker), 7 bits per byte."""
    d = int(d)
    u = (((d << 1) ^ (d >> 63)) & M64) + 1
    out = bytearray()
    while u >= 0x80:
        out.append((u & 0x7F) | 0x80)
        u >>= 7
    out.append(u)
    return bytes(out)


def regular_stream(ops, n, tokens):
    """The regular stream of n points: tokens[o][i] = bytes of op o's token of point i."""
    return b"".join(tokens[o][i] for i in range(n) for o in range(len(ops)))


class Parsed:
    """A chunk's regular stream, point by point: start[i] (payload offset), size[i], lead[i] (bytes of the varints the point begins
    with), changed[i] (a '11' token of the point opens a window different from the one in effect for its op), kinds[g][i] and
    values[g] per Gorilla op g, wins[i] = the windows of all Gorilla ops BEHIND point i, end = where the stream ends."""


def parse_regular(payload, ops, n):
    buf = bytes(payload)
    gops = [o for o, k in enumerate(ops) if k == "g"]
    k0 = next((o for o, k in enumerate(ops) if k != "v"), len(ops))
    P = Parsed()
    P.start, P.size, P.lead, P.changed, P.wins = [], [], [], [], []
    P.kinds = [[] for _ in gops]
    vals = [[] for _ in gops]
    win = [None] * len(gops)
    prev = [0] * len(gops)
    pos = 0
    for i in range(n):
        p0, chg, lead = pos, False, 0
        for o, kind in enumerate(ops):
            if kind == "v":
                k = 0
                while True:
                    if pos + k >= len(buf):
                        raise GorillaError("truncated", "varint at byte %d" % pos)
                    k += 1
                    if buf[pos + k - 1] < 0x80:
                        break
                    if k == 10:
                        raise GorillaError("corrupt", "varint of more than 10 bytes at byte %d" % pos)
                pos += k
                if o < k0:
                    lead += k
            elif kind == "g":
                g = gops.index(o)
                size, x, tk, nw = read_token(buf, pos, i == 0, win[g])
                if tk == "11" and nw != win[g]:
                    chg = True
                win[g] = nw
                prev[g] = x if tk == "first" else prev[g] ^ x
                vals[g].append(prev[g])
                P.kinds[g].append(tk)
                pos += size
            else:
                if pos + kind[1] > len(buf):
                    raise GorillaError("truncated", "raw field at byte %d" % pos)
                pos += kind[1]
        P.start.append(p0)
        P.size.append(pos - p0)
        P.lead.append(lead)
        P.changed.append(chg)
        P.wins.append(tuple(win))
    P.values = [np.array(v, dtype=np.uint64) for v in vals]
    P.end = pos
    return P


class Piece:
    def __init__(self, index, first_point, npts, changes, window_front):
        self.index, self.first_point, self.npts, self.changes, self.window_front = index, first_point, npts, changes, window_front
        self.rounds = 1 + changes   # tables built for the piece when the entry guess is right: one, plus one per changing point


def serial_expected(payload, a0, ops, n, parsed=None):
    """-> (serial, reason, pieces). MODE 2's hand-over rules for a well-formed chunk whose payload lies at address = a0 (mod 16):
    * pieces of 1024 bytes at 16-byte aligned addresses: piece p holds the addresses [1024 p, 1024 p + 1024) counted from
      (payload address - a0); a piece owns the points that BEGIN in it ("chain 1", entry / pts0);
    * a piece is redone in rounds: a round ends behind a point whose '11' token opens a different window, and after the round
      that makes `rounds >= kSwMaxRounds` the chunk is handed over -- unless that point was the piece's (or the chunk's) last,
      in which case the loop has left already ("MODE 2, rounds": `if (flag == 0u || wx >= kSwPiece || wj >= limit) break;` comes
      before `if (rounds >= kSwMaxRounds)`). So: serial iff the 40th changing point of a piece is not the last point it owns;
    * a point of more than kSwMaxPointBytes bytes gets no jump-table entry (`len <= kSwMaxPointBytes`);
    * neither does a point whose leading varints end more than 64 bytes behind the first byte of the point's 16-byte unit
      (make_jt_gor: `rel_add(i, m ? ctz(m) + 1 : 64)` over the 64 end bits R[1]:R[0]).
    pieces[k].window_front = the windows (one per Gorilla op) in effect in front of the piece's first point."""
    P = parsed or parse_regular(payload, ops, n)
    pieces, serial, reason = [], 0, ""
    i = 0
    while i < n:
        p = (a0 + P.start[i]) // PIECE
        j = i
        while j < n and (a0 + P.start[j]) // PIECE == p:
            j += 1
        changes = 0
        for q in range(i, j):
            v = a0 + P.start[q]
            if P.size[q] > MAX_POINT_BYTES and not serial:
                serial, reason = 1, "point %d has %d bytes" % (q, P.size[q])
            if (v & 15) + P.lead[q] > LEAD_VARINT_SPAN and not serial:
                serial, reason = 1, "point %d: leading varints end %d bytes into its unit" % (q, (v & 15) + P.lead[q])
            if P.changed[q]:
                changes += 1
                if changes == MAX_ROUNDS and q != j - 1 and not serial:
                    serial, reason = 1, "piece %d: %d window changes, the last at point %d of [%d, %d)" % (p, changes, q, i, j)
        front = tuple([None] * len(P.values)) if i == 0 else P.wins[i - 1]
        pieces.append(Piece(p, i, j - i, changes, front))
        i = j
    return serial, reason, pieces
