"""Reject parity, enumerated: a TABLE of malformed and non-canonical streams -- not random damage --
decoded by the HIP path and by the compiled reference (oracle/_ref). The decision (accept / reject) and, when the stream is
accepted, every output byte must be the reference's.

What the reference's decoder checks, and where:
  decodeVarint (include/cloudini_lib/encoding_utils.hpp:98-148): empty input, truncated input, shift >= 64, payload > 1 at
      shift 63, value 0 ("unexpected NaN marker"); non-canonical paddings (0x80 groups, a final 0x00) are ACCEPTED
  decodeV5AdaptiveIntSection (src/v5_codec.cpp:764-879): mode byte, Palette count / table / index >= count / short index
      bytes, run records past n, run counts that leave bytes over, truncated sections
  DecodeV5Stage1Chunk (src/v5_codec.cpp:984-1012): payload bytes left over behind the last section
The table: varints of 1..10 bytes for the same value (canonical and padded by 1..n zero groups), 11 bytes (shift >= 64), the
bit-63 overflow, the overlong zero, a stream cut inside a token at every byte -- each in a FloatN lane (k_decode_points_w), a
scalar lossy lane and a 64-bit integer lane (k_decode_stream_w, MSB mode) and next to a raw field (byte automaton + bitmap
mode); each at the chunk's first token, at tokens around the decoder's piece boundaries (992 and 1024 bytes), in the middle and
at the chunk's last token, in a full first chunk and in the ragged last one. Then the four section modes: headers and bodies.
"""
import numpy as np
import pytest

import cases
import lz4_block_rules as R
import lz4_body as B
from cloudini_amd import synth
from cloudini_amd.schema import CompressionOption, FieldType as F

pytestmark = pytest.mark.gpu

FILL = 0x5A


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _split_chunks(stream):
    pos, res = 0, []
    while pos < len(stream):
        size = int(np.frombuffer(stream[pos:pos + 4].tobytes(), "<u4")[0])
        res.append(stream[pos + 4:pos + 4 + size].copy())
        pos += 4 + size
    return res


def _reframe(payloads):
    out = []
    for p in payloads:
        out.append(np.frombuffer(np.uint32(len(p)).tobytes(), np.uint8))
        out.append(np.asarray(p, dtype=np.uint8))
    return np.concatenate(out)


def _uval(token) -> int:
    u = 0
    for k, b in enumerate(token):
        u |= (int(b) & 0x7F) << (7 * k)
    return u


def _encode_uval(u: int, length: int) -> np.ndarray:
    """`u` as a varint of exactly `length` bytes: canonical when length is the shortest, otherwise padded with zero groups
    (0x80 ... 0x00), which decodeVarint accepts."""
    groups = []
    v = u
    while True:
        groups.append(v & 0x7F)
        v >>= 7
        if v == 0:
            break
    assert len(groups) <= length
    groups += [0] * (length - len(groups))
    out = [g | 0x80 for g in groups[:-1]] + [groups[-1]]
    return np.array(out, dtype=np.uint8)


def _variants(token):
    """(name, replacement bytes) for one varint token of the stream."""
    u = _uval(token)
    n0 = 1
    while (u >> (7 * n0)) != 0:
        n0 += 1
    out = []
    for length in range(n0, 11):
        out.append((f"len{length}" + ("" if length == n0 else f"_pad{length - n0}"), _encode_uval(u, length)))
    out.append(("shift64_11_bytes", np.array([0x80 | (u & 0x7F)] + [0x80] * 9 + [0x01], dtype=np.uint8)))
    out.append(("shift64_12_bytes", np.array([0x80 | (u & 0x7F)] + [0x80] * 10 + [0x00], dtype=np.uint8)))
    out.append(("bit63_payload_2", np.array([0x80 | (u & 0x7F)] + [0x80] * 8 + [0x02], dtype=np.uint8)))
    out.append(("bit63_payload_1", np.array([0x80 | (u & 0x7F)] + [0x80] * 8 + [0x01], dtype=np.uint8)))  # legal: bit 63 set
    out.append(("bit63_payload_7f", np.array([0xFF] * 9 + [0x7F], dtype=np.uint8)))
    for length in (2, 3, 4, 5, 10):
        out.append((f"overlong_zero_{length}", np.array([0x80] * (length - 1) + [0x00], dtype=np.uint8)))
    return out


class _Checker:
    """One codec per layout, kept across the table's cases (it must stay usable behind every reject)."""

    def __init__(self, reflib, info):
        from cloudini_amd import native
        self.native = native
        self.reflib = reflib
        self.info = info
        self.codec = native.Codec(native.Plan(info))
        self.accepted = 0
        self.rejected = 0
        self.lz4_routed = 0

    def check(self, stream, n, what):
        info = self.info.copy(width=n, height=1)
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        try:
            want = self.reflib.decode_noheader(info, stream, fill=FILL)
            ref_ok = True
        except Exception:
            want, ref_ok = None, False
        out = np.full(max(1, n * info.point_step), FILL, dtype=np.uint8)
        try:
            got = self.codec.decode_host([stream], [n], out=out)[0]
            gpu_ok = True
        except self.native.CloudiniHipError as e:
            assert e.code == -6, (what, e)
            gpu_ok = False
        assert gpu_ok == ref_ok, f"{what}: reference {'accepts' if ref_ok else 'rejects'}, HIP path {'accepts' if gpu_ok else 'rejects'}"
        if ref_ok:
            assert np.array_equal(got, want), f"{what}: first difference at byte {int(np.nonzero(got != want)[0][0])}"
            self.accepted += 1
        else:
            self.rejected += 1
        self.check_lz4_route(info, stream, n, what)

    def check_lz4_route(self, info, stream, n, what):
        """The same row through cldn_hip_decode_lz4 when the stream's chunk chain parses (its sizes add up): every payload as
        liblz4's block (the strict rules accept those, so the reference is the exact judge here as well)."""
        pos, payloads = 0, []
        while pos + 4 <= len(stream):
            size = int.from_bytes(stream[pos:pos + 4].tobytes(), "little")
            if size > len(stream) - pos - 4:
                return
            payloads.append(stream[pos + 4:pos + 4 + size])
            pos += 4 + size
        if pos != len(stream):
            return
        body = B.frame([R.lz4_compress(p.tobytes()) for p in payloads])
        try:
            want = self.reflib.decode_noheader(info.copy(compression_opt=CompressionOption.LZ4), body, fill=FILL)
            ref_ok = True
        except Exception:
            want, ref_ok = None, False
        out = np.full(max(1, n * info.point_step), FILL, dtype=np.uint8)
        try:
            got = self.codec.decode_lz4_host([body], [n], out=out)[0]
            gpu_ok = True
        except self.native.CloudiniHipError as e:
            assert e.code == -6, (what, e)
            gpu_ok = False
        assert gpu_ok == ref_ok, f"{what}, as an LZ4 body: reference {'accepts' if ref_ok else 'rejects'}, HIP path {'accepts' if gpu_ok else 'rejects'}"
        if ref_ok:
            assert np.array_equal(got, want), f"{what}, as an LZ4 body: first difference at byte {int(np.nonzero(got != want)[0][0])}"
        self.lz4_routed += 1

    def close(self):
        self.codec.close()


def _layout(kind, n, seed=5):
    rs = np.random.RandomState(seed)
    if kind == "floatn":         # k_decode_points_w
        info, data = synth.lidar_xyz(n, seed=seed)
        return info, data, lambda op: True
    if kind == "floatn_v5":      # the same with a Palette section behind the regular stream
        info, data = synth.lidar_xyzi(n, seed=seed)
        return info, data, lambda op: True
    if kind == "scalar_lossy":   # stream kernel, MSB mode, 64-bit tokens
        fields = [("t", 0, F.FLOAT64, 1e-6), ("a", 8, F.FLOAT32, 0.01)]
        cols = {"t": np.cumsum(rs.uniform(0, 1e-3, n)) + 1.7e9, "a": np.cumsum(rs.normal(0, 0.05, n)).astype(np.float32)}
        info = cases.make_info(fields, 12, n, version=4)
        return info, cases.pack(info, cols, n), lambda op: True
    if kind == "int64":          # FieldDecoderInt<int64_t> on the V4 wire
        fields = [("k", 0, F.INT64, None), ("j", 8, F.INT32, None)]
        cols = {"k": np.cumsum(rs.randint(-5000, 5000, n)).astype(np.int64), "j": np.cumsum(rs.randint(-50, 50, n)).astype(np.int32)}
        info = cases.make_info(fields, 12, n, version=4)
        return info, cases.pack(info, cols, n), lambda op: True
    if kind == "next_to_raw":    # a varint, then a raw 4-byte field: byte automaton + bitmap mode
        fields = [("x", 0, F.FLOAT32, 0.001), ("rgb", 4, F.FLOAT32, None)]
        cols = {"x": np.cumsum(rs.normal(0, 0.01, n)).astype(np.float32), "rgb": rs.randint(0, 1 << 24, n).astype(np.uint32).view(np.float32)}
        info = cases.make_info(fields, 8, n, version=4)
        return info, cases.pack(info, cols, n), lambda op: op == 0
    raise ValueError(kind)


def _token_spans(chunk, n_points, n_ops, is_varint, raw_size=4):
    """(start, end) of every varint token of the regular stream of one chunk (raw fields are stepped over)."""
    spans, pos = [], 0
    for _pt in range(n_points):
        for op in range(n_ops):
            if not is_varint(op):
                pos += raw_size
                continue
            start = pos
            while chunk[pos] & 0x80:
                pos += 1
            pos += 1
            spans.append((start, pos))
    return spans, pos


LANES = ["floatn", "floatn_v5", "scalar_lossy", "int64", "next_to_raw"]


@pytest.mark.parametrize("kind", LANES)
def test_varint_forms_in_every_lane_kind(reflib, kind):
    """Every form of the table replaces ONE token (the rest of the stream is the encoder's); positions: the chunk's first
    token, tokens around byte 992 / 1024 / 1984 / 2048 of the payload (the point and stream kernels' piece boundaries -- the
    payload's own misalignment shifts them by up to 15 bytes, so a window of tokens is taken), a token in the middle, the
    chunk's last token; in the full first chunk and in the ragged last chunk."""
    n = 32768 + 3000
    info, data, is_varint = _layout(kind, n)
    n_ops = {"floatn": 3, "floatn_v5": 3, "scalar_lossy": 2, "int64": 2, "next_to_raw": 2}[kind]
    ref_stream = reflib.encode_stage1(info, data)
    chunks = _split_chunks(ref_stream)
    assert len(chunks) == 2
    chk = _Checker(reflib, info)
    chk.check(ref_stream, n, "the encoder's own stream")
    for ci, n_chunk in ((0, 32768), (1, n - 32768)):
        ch = chunks[ci]
        spans, reg_end = _token_spans(ch, n_chunk, n_ops, is_varint)
        picks = {0, len(spans) - 1, len(spans) // 2}
        for boundary in (992, 1024, 1984, 2048):
            near = [k for k, (a, b) in enumerate(spans) if boundary - 20 <= a <= boundary + 4]
            picks.update(near[::3])
        for k in sorted(picks):
            a, b = spans[k]
            tok = ch[a:b]
            if tok[0] == 0:      # (a NaN marker: not a varint)
                continue
            forms = _variants(tok)
            if k not in (0, len(spans) - 1, len(spans) // 2):
                forms = [f for f in forms if f[0] in ("len5_pad4", "len5_pad3", "len5_pad2", "len5_pad1", "len5", "len10_pad9", "len10_pad8",
                                                      "shift64_11_bytes", "bit63_payload_2", "overlong_zero_2", "overlong_zero_4")
                         or f[0].startswith("len4") or f[0].startswith("len3")]
            for name, rep in forms:
                bad = [c for c in chunks]
                bad[ci] = np.concatenate([ch[:a], rep, ch[b:]])
                chk.check(_reframe(bad), n, f"{kind}, chunk {ci}, token {k} at byte {a}: {name}")
        # the stream cut inside / behind tokens: the chunk's payload ends after every byte of its last three tokens
        if reg_end == len(ch):   # (no sections behind the regular stream)
            a3 = spans[-3][0]
            for cut in range(a3, len(ch)):
                bad = [c for c in chunks]
                bad[ci] = ch[:cut]
                chk.check(_reframe(bad), n, f"{kind}, chunk {ci}: payload cut at byte {cut} of {len(ch)}")
            # ... and a last token made longer, then cut at each of its bytes
            a, b = spans[-1]
            if ch[a] != 0:
                long_tok = _encode_uval(_uval(ch[a:b]), 10)
                for keep in range(1, 10):
                    bad = [c for c in chunks]
                    bad[ci] = np.concatenate([ch[:a], long_tok[:keep]])
                    chk.check(_reframe(bad), n, f"{kind}, chunk {ci}: last token of 10 bytes cut after {keep}")
    assert chk.accepted > 20 and chk.rejected > 20, (chk.accepted, chk.rejected)
    assert chk.lz4_routed == chk.accepted + chk.rejected                     # (every row of this table keeps the chain whole)
    chk.close()


# ---- sections ----------------------------------------------------------------------------------------------------------
def _uvarint(u: int) -> bytes:
    out = []
    while u > 0x7F:
        out.append((u & 0x7F) | 0x80)
        u >>= 7
    out.append(u)
    return bytes(out)


def _section_cases(mode, n):
    """(name, section bytes) for an integer-only UINT16 cloud of n points whose values are i % 5 * 3 (Palette, Rle) or
    i // 4 (DeltaRle, DeltaVarint): hand-written sections, well formed first, then one defect each."""
    out = []
    if mode == 1:   # Palette: [1][u16 count][count x u16][bit-packed indexes]
        vals = [0, 3, 6, 9, 12]
        bits = 3
        idx = [(i % 5) for i in range(n)]
        packed = bytearray((bits * n + 7) // 8)
        for i, v in enumerate(idx):
            for bb in range(bits):
                if (v >> bb) & 1:
                    packed[(i * bits + bb) >> 3] |= 1 << ((i * bits + bb) & 7)
        head = bytes([1]) + (5).to_bytes(2, "little") + b"".join(v.to_bytes(2, "little") for v in vals)
        good = head + bytes(packed)
        out.append(("good", good))
        bad_idx = bytearray(packed)
        bad_idx[0] |= 0x07                                             # index 7 >= count 5 at point 0
        out.append(("index_ge_count_first_point", head + bytes(bad_idx)))
        bad_idx = bytearray(packed)
        last_bit = bits * (n - 1)
        for bb in range(bits):
            bad_idx[(last_bit + bb) >> 3] |= 1 << ((last_bit + bb) & 7)
        out.append(("index_ge_count_last_point", head + bytes(bad_idx)))
        out.append(("count_0", bytes([1]) + (0).to_bytes(2, "little") + bytes(packed)))
        out.append(("count_larger_than_table", bytes([1]) + (40000).to_bytes(2, "little") + good[3:]))
        out.append(("table_cut", good[:6]))
        out.append(("header_cut_1", good[:1]))
        out.append(("header_cut_2", good[:2]))
        out.append(("index_bytes_short_by_1", good[:-1]))
        out.append(("index_bytes_long_by_1", good + b"\x00"))
        out.append(("count_1_no_index_bytes", bytes([1]) + (1).to_bytes(2, "little") + (7).to_bytes(2, "little")))
        out.append(("count_1_with_index_bytes", bytes([1]) + (1).to_bytes(2, "little") + (7).to_bytes(2, "little") + bytes(packed)))
    elif mode == 2:  # Rle: [2][u32 runs] runs x {u16 raw, uvarint run_len}
        runs = [(7 + (r % 3), 10) for r in range(n // 10)] + ([(1, n % 10)] if n % 10 else [])
        def build(rs_, count=None):
            body = b"".join(v.to_bytes(2, "little") + _uvarint(l) for v, l in rs_)
            return bytes([2]) + (len(rs_) if count is None else count).to_bytes(4, "little") + body
        out.append(("good", build(runs)))
        out.append(("run_past_n", build(runs[:-1] + [(runs[-1][0], runs[-1][1] + 1)])))
        out.append(("runs_short_of_n", build(runs[:-1])))
        out.append(("count_one_less_than_written", build(runs, len(runs) - 1)))
        out.append(("count_one_more_than_written", build(runs, len(runs) + 1)))
        out.append(("run_len_0", build([(5, 0)] + runs)))
        out.append(("run_len_padded", bytes([2]) + len(runs).to_bytes(4, "little") + runs[0][0].to_bytes(2, "little") + bytes([0x80 | runs[0][1], 0x80, 0x00]) +
                    b"".join(v.to_bytes(2, "little") + _uvarint(l) for v, l in runs[1:])))
        out.append(("run_len_11_bytes", bytes([2]) + len(runs).to_bytes(4, "little") + runs[0][0].to_bytes(2, "little") + bytes([0x8A] + [0x80] * 9 + [0x01]) +
                    b"".join(v.to_bytes(2, "little") + _uvarint(l) for v, l in runs[1:])))
        out.append(("cut_in_header", build(runs)[:3]))
        out.append(("cut_in_a_value", build(runs)[:6]))
        out.append(("cut_in_the_last_run", build(runs)[:-1]))
        out.append(("first_run_covers_all", build([(9, n)])))
        out.append(("first_run_2_pow_32", build([(9, 1 << 32)])))
    elif mode == 3:  # DeltaRle: [3][u32 runs] runs x {varint diff, uvarint run_len}
        def zz(v):
            return _uvarint(((v << 1) ^ (v >> 63)) + 1)
        runs = [(3, 1)] + [(1, 1), (0, 3)] * ((n - 1) // 4)
        total = sum(l for _d, l in runs)
        if total < n:
            runs.append((0, n - total))
        def build(rs_, count=None):
            body = b"".join(zz(d) + _uvarint(l) for d, l in rs_)
            return bytes([3]) + (len(rs_) if count is None else count).to_bytes(4, "little") + body
        out.append(("good", build(runs)))
        out.append(("run_past_n", build(runs[:-1] + [(runs[-1][0], runs[-1][1] + 1)])))
        out.append(("runs_short_of_n", build(runs[:-1])))
        out.append(("count_one_more_than_written", build(runs, len(runs) + 1)))
        out.append(("diff_is_nan_marker", bytes([3]) + len(runs).to_bytes(4, "little") + b"\x00" + _uvarint(1) + b"".join(zz(d) + _uvarint(l) for d, l in runs[1:])))
        out.append(("diff_padded", bytes([3]) + len(runs).to_bytes(4, "little") + bytes([0x80 | 7, 0x80, 0x00]) + _uvarint(1) + b"".join(zz(d) + _uvarint(l) for d, l in runs[1:])))
        out.append(("diff_overlong_zero", bytes([3]) + len(runs).to_bytes(4, "little") + bytes([0x80, 0x00]) + _uvarint(1) + b"".join(zz(d) + _uvarint(l) for d, l in runs[1:])))
        out.append(("run_len_0", build([(2, 0)] + runs)))
        out.append(("cut_in_the_last_run", build(runs)[:-1]))
        out.append(("cut_in_header", build(runs)[:4]))
    else:            # DeltaVarint: [0] n x varint diff
        def zz(v):
            return _uvarint(((v << 1) ^ (v >> 63)) + 1)
        diffs = [5] + [(1 if i % 4 == 0 else 0) for i in range(1, n)]
        good = bytes([0]) + b"".join(zz(d) for d in diffs)
        out.append(("good", good))
        out.append(("one_token_short", good[:-1]))
        out.append(("one_token_more", good + zz(0)))
        out.append(("first_padded_to_5", bytes([0]) + bytes(_encode_uval(11, 5)) + good[2:]))
        out.append(("first_padded_to_10", bytes([0]) + bytes(_encode_uval(11, 10)) + good[2:]))
        out.append(("first_is_nan_marker", bytes([0, 0]) + good[2:]))
        out.append(("first_overlong_zero", bytes([0, 0x80, 0x00]) + good[2:]))
        out.append(("first_11_bytes", bytes([0]) + bytes([0x8B] + [0x80] * 9 + [0x01]) + good[2:]))
        out.append(("first_bit63_payload_2", bytes([0]) + bytes([0x8B] + [0x80] * 8 + [0x02]) + good[2:]))
        mid = 1 + (n // 2)
        out.append(("middle_padded_to_3", good[:mid] + bytes(_encode_uval(good[mid], 3)) + good[mid + 1:]))
        out.append(("last_padded_to_4", good[:-1] + bytes(_encode_uval(good[-1], 4))))
        out.append(("last_cut", good[:-1] + bytes([0x80 | good[-1]])))
        out.append(("mode_byte_4", bytes([4]) + good[1:]))
        out.append(("mode_byte_255", bytes([255]) + good[1:]))
        out.append(("empty_section", b""))
    return out


@pytest.mark.parametrize("n", [4133, 32768, 600])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_section_headers_and_bodies(reflib, mode, n):
    """An integer-only UINT16 cloud (one section per chunk, no regular stream): hand-written sections of each mode, well
    formed and with one defect each; for a single chunk and behind a first chunk that is well formed."""
    info, _ = cases.int_only(np.zeros(n, dtype=np.uint16), F.UINT16)
    chk = _Checker(reflib, info)
    table = _section_cases(mode, n)
    assert table[0][0] == "good"
    for name, sec in table:
        chk.check(_reframe([np.frombuffer(sec, dtype=np.uint8)]), n, f"mode {mode}, n {n}: {name}")
    assert chk.accepted >= 1 and chk.rejected >= 4, (chk.accepted, chk.rejected)
    chk.close()
    if n == 600:   # the same defects in the ragged SECOND chunk of a two-chunk cloud
        n2 = 32768 + n
        info2, _ = cases.int_only(np.zeros(n2, dtype=np.uint16), F.UINT16)
        chk = _Checker(reflib, info2)
        first = np.frombuffer(_section_cases(mode, 32768)[0][1], dtype=np.uint8)
        for name, sec in table:
            chk.check(_reframe([first, np.frombuffer(sec, dtype=np.uint8)]), n2, f"mode {mode}, second chunk of {n} points: {name}")
        chk.close()


@pytest.mark.parametrize("kind", ["xyzi", "velodyne"])
def test_sections_behind_a_regular_stream(reflib, kind):
    """The section defects behind a FloatN regular stream (the layouts of BASELINE configs[1] and [3]): the point kernel folds a
    well-formed Palette in; everything else must fall through to the checks of the section decoders."""
    n = 32768 + 2500
    info, data = (synth.lidar_xyzi if kind == "xyzi" else synth.velodyne_xyzir)(n, seed=21)
    stream = reflib.encode_stage1(info, data)
    chunks = _split_chunks(stream)
    chk = _Checker(reflib, info)
    chk.check(stream, n, "the encoder's own stream")
    n_ops = 3 if kind == "xyzi" else 4
    for ci, n_chunk in ((0, 32768), (1, n - 32768)):
        ch = chunks[ci]
        _spans, reg_end = _token_spans(ch, n_chunk, n_ops, lambda op: True)
        sec = ch[reg_end:]
        forms = []
        if sec[0] == 1:   # Palette (intensity)
            count = int(sec[1]) | (int(sec[2]) << 8)
            bits = max(1, int(count - 1).bit_length()) if count > 1 else 0
            forms.append(("palette count + 1", np.concatenate([sec[:1], np.frombuffer((count + 1).to_bytes(2, "little"), np.uint8), sec[3:]])))
            forms.append(("palette count - 1", np.concatenate([sec[:1], np.frombuffer((count - 1).to_bytes(2, "little"), np.uint8), sec[3:]])))
            forms.append(("palette count 0", np.concatenate([sec[:1], np.zeros(2, np.uint8), sec[3:]])))
            if count < (1 << bits):   # an index value the table does not have
                s2 = sec.copy()
                s2[3 + 2 * count:3 + 2 * count + 2] = 0xFF
                forms.append(("palette index >= count", s2))
            s2 = sec.copy()
            s2[3:5] = [0x34, 0x12]
            forms.append(("palette table value changed (legal)", s2))
        forms.append(("mode byte 7", np.concatenate([[np.uint8(7)], sec[1:]])))
        forms.append(("one byte short", sec[:-1]))
        forms.append(("one byte over", np.concatenate([sec, [np.uint8(0)]])))
        forms.append(("three bytes over", np.concatenate([sec, np.array([1, 0, 0], np.uint8)])))
        forms.append(("section missing", sec[:0]))
        forms.append(("only the mode byte", sec[:1]))
        for name, s2 in forms:
            bad = [c for c in chunks]
            bad[ci] = np.concatenate([ch[:reg_end], np.asarray(s2, dtype=np.uint8)])
            chk.check(_reframe(bad), n, f"{kind}, chunk {ci}: {name}")
    assert chk.rejected >= 8
    chk.close()


@pytest.mark.parametrize("what", ["zero_size_chunk", "size_past_end", "size_0xffffffff", "chunk_missing", "chunk_extra", "prefix_cut",
                                  "empty_stream", "n_0_with_bytes"])
def test_chunk_framing(reflib, what):
    """[u32 size][payload] framing (src/cloudini.cpp:635-684): sizes that lie, chunks that are missing or left over."""
    n = 32768 + 100
    info, data = synth.lidar_xyz(n, seed=3)
    stream = reflib.encode_stage1(info, data)
    chunks = _split_chunks(stream)
    chk = _Checker(reflib, info)
    if what == "zero_size_chunk":
        s = _reframe([chunks[0], np.zeros(0, np.uint8)])
    elif what == "size_past_end":
        s = stream.copy()
        s[0:4] = np.frombuffer(np.uint32(len(stream)).tobytes(), np.uint8)
    elif what == "size_0xffffffff":
        s = stream.copy()
        s[0:4] = 0xFF
    elif what == "chunk_missing":
        s = _reframe(chunks[:1])
    elif what == "chunk_extra":
        s = _reframe(chunks + [chunks[1]])
    elif what == "prefix_cut":
        s = stream[: 4 + len(chunks[0]) + 2]
    elif what == "empty_stream":
        s = np.zeros(0, np.uint8)
    else:
        chk.close()
        info0 = info.copy(width=0, height=1)
        chk = _Checker(reflib, info0)
        chk.check(_reframe(chunks[:1]), 0, what)
        chk.close()
        return
    chk.check(s, n, what)
    chk.close()
