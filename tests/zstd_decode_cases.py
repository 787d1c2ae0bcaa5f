"""The inputs of the ZSTD decoder's tests (tests/test_zstd_lit_rules.py, test_zstd_walk_cpu.py, test_gpu_zstd_decode.py):
  a  grid_frames()     the model writer's frame of every payload of tests/zstd_payload_grid.py
  b  libzstd_frames()  frames made by the system libzstd over sources x compression parameters
  c  hand_frames()     frames built from the model's pieces for what no compressor here writes
  d  damaged()         every single-byte change (255 values) of the header bytes the walk reads, truncations, random byte damage
Every entry is (name, frame bytes, capacity); the verdicts are tests/zstd_lit_rules.py's. Computed once and shared."""
import ctypes as C
import functools

import numpy as np

import zstd_lit_model as M
import zstd_lit_rules as R
import zstd_payload_grid as G

_z = None
C_LEVEL, C_WINDOW_LOG, C_MIN_MATCH, C_STRATEGY, C_CHECKSUM = 100, 101, 105, 107, 201


def zstd():
    global _z
    if _z is None:
        _z = C.CDLL("libzstd.so.1")
        _z.ZSTD_decompress.restype = C.c_size_t
        _z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        _z.ZSTD_isError.argtypes = [C.c_size_t]
        _z.ZSTD_compressBound.restype = C.c_size_t
        _z.ZSTD_compressBound.argtypes = [C.c_size_t]
        _z.ZSTD_createCCtx.restype = C.c_void_p
        _z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
        _z.ZSTD_CCtx_setParameter.restype = C.c_size_t
        _z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _z.ZSTD_compress2.restype = C.c_size_t
        _z.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    return _z


def libzstd_decompress(frame: bytes, capacity: int):
    """-> the content, or None when ZSTD_decompress with room for exactly `capacity` bytes returns an error"""
    z = zstd()
    frame = bytes(frame)
    out = C.create_string_buffer(max(1, capacity))
    r = z.ZSTD_decompress(out, capacity, frame, len(frame))
    return None if z.ZSTD_isError(r) else out.raw[:r]


def libzstd_compress(payload: bytes, params) -> bytes:
    z = zstd()
    cctx = z.ZSTD_createCCtx()
    try:
        for k, v in params:
            assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(cctx, k, v))
        cap = z.ZSTD_compressBound(len(payload))
        out = C.create_string_buffer(max(1, cap))
        r = z.ZSTD_compress2(cctx, out, cap, payload, len(payload))
        assert not z.ZSTD_isError(r)
        return out.raw[:r]
    finally:
        z.ZSTD_freeCCtx(cctx)


# ---- a ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def grid_frames():
    out = []
    for c in G.grid():
        for i, row in enumerate(G.model(c)):
            for j, (payload, frame, _trace) in enumerate(row):
                out.append((f"{c.name}/{i}.{j}", frame.tobytes(), payload.size, payload.tobytes()))
    return out


# ---- b ---------------------------------------------------------------------------------------------------------------------------
LEVEL1 = ((C_LEVEL, 1),)
SMALL_BLOCKS = ((C_LEVEL, 1), (C_WINDOW_LOG, 10), (C_MIN_MATCH, 7), (C_STRATEGY, 1))
SIZES = [0, 1, 63, 64, 255, 256, 1023, 131071, 131072, 131073]


def sources():
    geo = np.minimum(np.random.default_rng(1).geometric(0.08, 300000) - 1, 255).astype(np.uint8)
    zipf = (np.random.default_rng(1).zipf(1.3, 300000) % 256).astype(np.uint8)
    return {"geometric": geo.tobytes(), "zipf": zipf.tobytes(), "constant": b"\x37" * 300000,
            "random": np.random.default_rng(2).integers(0, 256, 300000, dtype=np.uint8).tobytes()}


@functools.lru_cache(None)
def libzstd_frames():
    """-> [(name, frame, capacity, payload)]"""
    out = []
    src = sources()
    for sname in ("geometric", "zipf"):
        for pname, params in (("level1", LEVEL1), ("small_blocks", SMALL_BLOCKS)):
            out.append((f"{sname}/{pname}/300000", libzstd_compress(src[sname], params), 300000, src[sname]))
    # (SMALL_BLOCKS over a shorter piece: few enough blocks for a frame to be literal-only as a whole)
    for sname in ("geometric", "zipf"):
        for n in (2048, 3072, 5120, 8192):
            for at in (0, 7000, 50000):
                p = src[sname][at:at + n]
                out.append((f"{sname}/small_blocks/{n}@{at}", libzstd_compress(p, SMALL_BLOCKS), n, p))
    for sname in ("geometric", "zipf", "constant", "random"):
        for n in SIZES:
            p = src[sname][:n]
            out.append((f"{sname}/level1/{n}", libzstd_compress(p, LEVEL1), n, p))
    out.append(("geometric/checksum/1023", libzstd_compress(src["geometric"][:1023], LEVEL1 + ((C_CHECKSUM, 1),)), 1023,
                src["geometric"][:1023]))
    return out


# ---- c ---------------------------------------------------------------------------------------------------------------------------
def frame_header(content=None, *, single=True, fcs_bytes=4, window_byte=0x50):
    """every form without dictionary and checksum; fcs_bytes 0 needs single=False"""
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    assert fcs_bytes != 0 or not single
    assert fcs_bytes != 1 or single
    fhd = (flag << 6) | (int(single) << 5)
    out = b"\x28\xb5\x2f\xfd" + bytes([fhd])
    if not single:
        out += bytes([window_byte])
    if fcs_bytes:
        out += (content - (256 if fcs_bytes == 2 else 0)).to_bytes(fcs_bytes, "little")
    return out


def huf_pieces(data: np.ndarray, four: bool, lens=None):
    """-> (tree description, jump table + streams, lens, codes) of data as one literals section"""
    if lens is None:
        lens = M.code_lengths(np.bincount(data, minlength=256))
    codes, max_len = M.code_values(lens)
    desc = M.tree_description(lens, max_len)
    n = data.size
    if four:
        seg = (n + 3) // 4
        streams = [M.stream_bytes(data[k * seg:min(n, (k + 1) * seg)], lens, codes) for k in range(4)]
        body = b"".join(len(s).to_bytes(2, "little") for s in streams[:3]) + b"".join(streams)
    else:
        body = M.stream_bytes(data, lens, codes)
    return desc, body, lens


def lit_header(lit_type: int, regen: int, comp: int, four: bool) -> bytes:
    _form, h = M.literals_header(regen, comp, four)
    return bytes([(h[0] & ~3) | lit_type]) + h[1:]


def huf_block(data, last, four, *, treeless_lens=None, direct=None):
    """a Compressed block: literals type 2 (or 3 with the lengths of an earlier block), the sequences byte 0"""
    desc, body, _lens = huf_pieces(data, four, treeless_lens)
    if direct is not None:
        desc = direct
    if treeless_lens is not None:
        sec = lit_header(3, data.size, len(body), four) + body
    else:
        sec = lit_header(2, data.size, len(desc) + len(body), four) + desc + body
    sec += b"\x00"
    return M.block_header(last, 2, len(sec)) + sec


def _short_header(lit_type: int, n: int, size_format: int) -> bytes:
    """the literals header of Raw / RLE literals: 5, 12 or 20 bits of size"""
    if size_format == 0:
        return bytes([(n << 3) | lit_type])
    return ((n << 4) | (size_format << 2) | lit_type).to_bytes(2 if size_format == 1 else 3, "little")


def raw_literals_block(data: bytes, last, size_format):
    n = len(data)
    h = _short_header(0, n, size_format)
    sec = h + data + b"\x00"
    return M.block_header(last, 2, len(sec)) + sec


def rle_literals_block(byte: int, n: int, last, size_format):
    h = _short_header(1, n, size_format)
    sec = h + bytes([byte]) + b"\x00"
    return M.block_header(last, 2, len(sec)) + sec


@functools.lru_cache(None)
def hand_frames():
    """-> [(name, frame, capacity, payload or None (None: the rules must not say OK))]"""
    out = []
    a = G.skewed(700, 11)
    b = G.skewed(300, 12, top=12)
    pa = a.tobytes()
    blk = M.block(a, True)[2]
    for single, fcs in ((True, 1), (True, 2), (True, 4), (True, 8), (False, 0), (False, 2), (False, 4), (False, 8)):
        if fcs == 1:
            d = a[:200]
            out.append(("header/single/1", frame_header(200, single=True, fcs_bytes=1) + M.block(d, True)[2], 200, d.tobytes()))
            continue
        out.append((f"header/{'single' if single else 'window'}/{fcs}", frame_header(700, single=single, fcs_bytes=fcs) + blk, 700, pa))
    out.append(("header/window/big", frame_header(700, single=False, fcs_bytes=4, window_byte=0x8f) + blk, 700, pa))
    # treeless behind a type-2 block: b's symbols all occur in a (checked), coded with a's lengths
    lens_a = M.code_lengths(np.bincount(a, minlength=256))
    assert all(lens_a[s] for s in np.unique(b))
    for four_a, four_b in ((True, True), (True, False), (False, True)):
        first = huf_block(a if four_a else a[:250], False, four_a)
        la = lens_a if four_a else M.code_lengths(np.bincount(a[:250], minlength=256))
        bb = b if four_a else b[np.isin(b, np.unique(a[:250]))]
        bb = bb[:250] if not four_b else bb
        pay = (a if four_a else a[:250]).tobytes() + bb.tobytes()
        out.append((f"treeless/{int(four_a)}{int(four_b)}", frame_header(len(pay)) + first + huf_block(bb, True, four_b, treeless_lens=la),
                    len(pay), pay))
    # a Raw block and an RLE block between the table and its treeless user
    pay = pa + b"\x05" * 40 + a[:30].tobytes() + b.tobytes()
    out.append(("treeless/behind_raw_rle", frame_header(len(pay)) + huf_block(a, False, True) + M.block_header(False, 1, 40) + b"\x05" +
                M.block_header(False, 0, 30) + a[:30].tobytes() + huf_block(b, True, True, treeless_lens=lens_a), len(pay), pay))
    out.append(("treeless/first", frame_header(b.size) + huf_block(b, True, True, treeless_lens=lens_a), b.size, None))
    # one stream at 255 symbols, four at 256
    out.append(("streams/one_255", frame_header(255) + huf_block(a[:255], True, False), 255, a[:255].tobytes()))
    out.append(("streams/four_256", frame_header(256) + huf_block(a[:256], True, True), 256, a[:256].tobytes()))
    out.append(("streams/one_700", frame_header(700) + huf_block(a, True, False), 700, pa))
    out.append(("streams/four_7", frame_header(7, single=False) + huf_block(a[:7], True, True), 7, a[:7].tobytes()))
    # (the same in a single-segment frame: the block is larger than the window its content size implies)
    out.append(("host/four_7_window", frame_header(7) + huf_block(a[:7], True, True), 7, None))
    # direct weights: 6 symbols with lengths 1 2 3 4 5 5 -> weights 5 4 3 2 1 (1), in symbol order
    d = np.repeat(np.arange(6, dtype=np.uint8), [64, 32, 16, 8, 4, 4])
    d = np.random.RandomState(5).permutation(d)
    lens_d = np.zeros(256, np.int64)
    lens_d[:6] = [1, 2, 3, 4, 5, 5]
    direct = bytes([127 + 5, 0x54, 0x32, 0x10])
    out.append(("direct/5", frame_header(d.size) + huf_block(d, True, False, direct=direct, treeless_lens=None), d.size, d.tobytes())
               if np.array_equal(M.code_lengths(np.bincount(d, minlength=256))[:6], lens_d[:6]) else None)
    # literals types 0 and 1, every size format; empty blocks in between
    body = (raw_literals_block(pa[:20], False, 0) + M.block_header(False, 0, 0) + raw_literals_block(pa[:300], False, 1) +
            raw_literals_block((pa * 8)[:5000], False, 3) + rle_literals_block(9, 31, False, 0) + M.block_header(False, 1, 0) + b"\x00" +
            rle_literals_block(10, 4000, False, 1) + rle_literals_block(11, 70000, True, 3))
    pay = pa[:20] + pa[:300] + (pa * 8)[:5000] + b"\x09" * 31 + b"\x0a" * 4000 + b"\x0b" * 70000
    out.append(("literals/raw_rle_forms", frame_header(len(pay)) + body, len(pay), pay))
    # what the device hands to the host or refuses, by construction
    out.append(("host/two_frames", M.frame(a) + M.frame(b), 1000, None))
    out.append(("host/skippable", b"\x50\x2a\x4d\x18\x04\x00\x00\x00abcd", 16, None))
    out.append(("host/sequences", frame_header(700) + blk[:-1] + b"\x01", 700, None))
    # more blocks than the frame's record limit behind a block whose tree description is damaged (its head byte 0): the device
    # judges the limit on a count that reads no tree description
    first = bytearray(huf_block(a, False, True))
    first[3 + 4] = 0                                      # (block header 3, literals header 4: the description's head byte)
    tail = b"".join(M.block_header(k == 39, 0, 1) + bytes([k]) for k in range(40))
    out.append(("host/many_blocks_bad_weights", frame_header(740) + bytes(first) + tail, 740, None))
    out.append(("corrupt/capacity", M.frame(a), 699, None))
    out.append(("corrupt/content_size", frame_header(701) + blk, 701, None))
    out.append(("corrupt/block_type", frame_header(700) + bytes([blk[0] | 6]) + blk[1:], 700, None))
    return [x for x in out if x is not None]


# ---- d ---------------------------------------------------------------------------------------------------------------------------
MAX_POSITIONS = 72   # (the frame header, the first blocks' headers, a tree description and its jump table lie within)


def header_positions(frame: bytes):
    """the bytes of the frame that the header walk reads -- frame header, every block and literals header, tree descriptions,
    jump tables, sequences bytes --, in frame order, the first MAX_POSITIONS of them"""
    note = {}
    R.walk(frame, 1 << 30, note=note)
    pos = sorted({at for a, b in note.get("headers", []) for at in range(a, min(b, len(frame)))})
    return pos[:MAX_POSITIONS]


@functools.lru_cache(None)
def damage_bases():
    g = {n: (f, c) for n, f, c, _p in grid_frames()}
    h = {n: (f, c) for n, f, c, _p in hand_frames()}
    l = {n: (f, c) for n, f, c, _p in libzstd_frames()}
    picks = [g[n] for n in sorted(g) if len(g[n][0]) < 1500][:3]
    picks += [h["treeless/11"], h["direct/5"], h["streams/one_255"], h["literals/raw_rle_forms"], h["header/window/2"]]
    picks += [l["geometric/level1/1023"], l["geometric/small_blocks/2048@0"]]
    return picks


@functools.lru_cache(None)
def damaged_base(i: int, random_seed: int = 0, random_per_base: int = 60):
    """-> [(name, frame, capacity)] of base i: EVERY single-byte change (all 255 other values) of every position of
    header_positions(), every truncation, and with a random_seed random damage of 1 to 3 bytes anywhere"""
    f, cap = damage_bases()[i]
    out = []
    for at in header_positions(f):
        for delta in range(1, 256):
            g = bytearray(f)
            g[at] ^= delta
            out.append((f"{i}/byte{at}^{delta:02x}", bytes(g), cap))
    for n in range(len(f)):
        out.append((f"{i}/cut{n}", f[:n], cap))
    if random_seed:
        rng = np.random.default_rng(random_seed * 1000 + i)
        for k in range(random_per_base):
            g = bytearray(f)
            for _ in range(int(rng.integers(1, 4))):
                g[int(rng.integers(0, len(g)))] = int(rng.integers(0, 256))
            out.append((f"{i}/random{k}", bytes(g), cap))
    return out


def damaged(random_seed: int = 0):
    """all bases"""
    return [c for i in range(len(damage_bases())) for c in damaged_base(i, random_seed)]
