"""Hand-built payloads for the device ZSTD writer with matches (cloudini_amd/csrc/zstd_seq_kernels.hip,
cldn_hip_codec_set_zstd_matches), one per code boundary, literals kind and size decision of it.

The tool is that of tests/zstd_payload_grid.py: raw-byte schemas, so a chunk's stage-1 payload IS its point bytes (RAW1: 32 KiB
chunks, RAW4 one full block, RAW5 a block and a quarter, RAW32 eight blocks).

A payload is composed of sequences (literal length, match length, offset) over incompressible filler: compose() copies the
match from `offset` bytes back and picks the bytes around it so that the match can neither start earlier nor go on. Whether the
device's match search -- 64 positions per step, one hash table per 8 KiB sub-range, the most recent position wins -- really
finds that match depends on where it lies; wanted() states it as a condition on the model's trace, and _find() moves the
payload byte by byte until the condition holds. The trace never supplies expected bytes: those are zstd_match_model.frame_info's.

What the format leaves out of reach here: offset codes 0 and 1 (offset values 1-3 are the repeat codes, which this writer does
not use; offset 1 has code 2), offset code 13 (a kept match has 12 bytes inside its 8192-byte sub-range, so its offset is 8180
at most and the offset value below 8192), match lengths above one sub-range, the 3-byte sequence count, a matched block that loses to Raw (see _build), and a block of 16 full match
lists of KEPT matches (a list holds 1024 matches in 8192 bytes, kept ones have 12 bytes: `dense_block` reaches what it says).
"""
from __future__ import annotations

import numpy as np

import zstd_lit_model as L
import zstd_match_model as M
import zstd_payload_grid as P
from zstd_payload_grid import CHUNK_POINTS, STEPS, Case, chunk_payloads, schema, skewed  # noqa: F401  (the tests' tools)

SUB, BLOCK, MIN = M.SUB, M.BLOCK, M.MIN_MATCH
ALIGNMENT_CASES = ["ll_15_to_18", "bits_mod8_0", "bits_mod8_7", "two_blocks_one_matched"]   # with `out` at every alignment

LL_EDGES = [15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 27, 28, 31, 32, 39, 40, 47, 48, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024,
            2047, 2048, 4095, 4096]
LL_LONG = [8191, 8192, 16383, 16384, 32767, 32768, 65535, 65536]
ML_EDGES = [34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 46, 47, 50, 51, 58, 59, 66, 67, 82, 83, 98, 99, 130, 131, 258, 259, 514, 515, 1026,
            1027, 2050, 2051, 4098, 4099]
OFFSETS = [1, 5, 13, 29, 61, 125, 253, 509, 1021, 2045, 4093, 8170]   # offset values 4 .. 8173: codes 2 .. 12


def rand(n: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)


def compose(seqs, seed: int, head: int = 0, tail: int = 16, filler=rand) -> np.ndarray:
    """head filler bytes, then per (ll, ml, off): ll filler bytes and ml bytes copied from off bytes back; tail filler bytes.
    The byte in front of a match differs from the one in front of its source, the byte behind it from the one behind its source."""
    n = head + sum(ll + ml for ll, ml, _ in seqs) + tail
    out = filler(n, seed).copy()
    at = head
    for ll, ml, off in seqs:
        at += ll
        assert at - off >= 0, (at, off)
        if ll and at - off - 1 >= 0 and out[at - 1] == out[at - off - 1]:
            out[at - 1] ^= 0x55
        for k in range(ml):                                 # (byte by byte: a source may overlap its copy)
            out[at + k] = out[at + k - off]
        at += ml
        if at < n and out[at] == out[at - off]:
            out[at] ^= 0xAA
    return out


def blocks_of(T):
    return [b for chunk in T for b in chunk]


def wanted(seqs, chunk: int = 0):
    """condition: every (ll, ml) is the literal and match length of a sequence of the case's chunk `chunk` (the offset is the
    parser's: the most recent position of equal bytes)"""
    def cond(T):
        have = set()
        for b in T[chunk]:
            if b.get("matched"):
                have.update((ll, ml) for ll, ml, _off in b["seqs"])
        missing = [s[:2] for s in seqs if tuple(s[:2]) not in have]
        assert not missing, missing
    return cond


def groups(values, k: int = 4):
    return [values[i:i + k] for i in range(0, len(values), k)]


def _trace(schema_name: str, clouds):
    T = []
    for cloud in clouds:
        for p in chunk_payloads(schema_name, cloud):
            t = []
            M.frame_info(p, t)
            T.append(t)
    return T


def _find(name, schema_name, make, cond, tries: int = 96) -> Case:
    """the first k for which make(k) -- a list of clouds -- meets cond on the model's trace"""
    last = None
    for k in range(tries):
        clouds = make(k)
        try:
            cond(_trace(schema_name, clouds))
        except AssertionError as e:
            last = e
            continue
        return Case(name, schema_name, clouds, cond)
    raise AssertionError(f"{name}: no payload met its condition: {last}")


def _pad_to(cloud: np.ndarray, step: int) -> np.ndarray:
    n = (cloud.size + step - 1) // step * step
    return np.concatenate([cloud, rand(n - cloud.size, 77)]) if n != cloud.size else cloud


def _build():
    out = []

    # ---- literal lengths each side of every code boundary; the long ones span sub-ranges (RAW32: up to 8 blocks per chunk,
    # a literal run of 65536 is half a block). The matches are 20 bytes from 300 back.
    for g in groups(LL_EDGES):
        seqs = [(70, 16, 90)] + [(ll, 20, 80) for ll in g]
        out.append(_find(f"ll_{g[0]}_to_{g[-1]}", "RAW1", lambda k, seqs=seqs: [compose(seqs, 100 + k, head=100 + k)], wanted(seqs[1:])))
    for ll in LL_LONG:
        s = [(70, 16, 66), (ll, 24, 80)]
        out.append(_find(f"ll_{ll}", "RAW4", lambda k, s=s: [_pad_to(compose(s, 200 + k, head=100 + k, tail=64), 4)], wanted(s[1:])))

    # ---- match lengths each side of every code boundary, up to what one sub-range yields
    for g in groups([ml for ml in ML_EDGES if ml <= 1027]):
        seqs = [(70, 16, 66)] + [(80, ml, 70) for ml in g]
        out.append(_find(f"ml_{g[0]}_to_{g[-1]}", "RAW1", lambda k, seqs=seqs: [compose(seqs, 300 + k, head=100 + k)], wanted(seqs[1:])))
    for ml in (2050, 2051, 4098):
        s = [(70, 16, 66), (30, ml, 80)]
        out.append(_find(f"ml_{ml}", "RAW1", lambda k, s=s: [compose(s, 400 + k, head=100 + k)], wanted(s[1:])))

    def cond_longest(T):   # the longest match of the window: all of a sub-range behind its first step
        assert max(ml for b in blocks_of(T) if b.get("matched") for _ll, ml, _off in b["seqs"]) >= SUB - 64 - 5, "no longest match"
    out.append(_find("ml_longest", "RAW1", lambda k: [np.full(SUB * 2, 7 + k, np.uint8)], cond_longest))

    # ---- one offset per offset code 2 .. 12, offset 1 (a run) among them. A far source survives in the hash table only if no
    # later position shares its hash: the filler of those cases is a run of zeros, which one long match of offset 1 swallows.
    def far(off, k):
        a = np.zeros(off + 200, np.uint8)
        src = k % 7
        a[src:src + 16] = 100 + np.arange(16)
        a[src + off:src + off + 16] = a[src:src + 16]
        return [a[:min(a.size, 2 * SUB)].copy()]
    for off in OFFSETS:
        def cond(T, off=off):
            assert any(o == off and M.highbit(o + 3) == M.highbit(off + 3) for b in blocks_of(T) if b.get("matched") for _l, _m, o in b["seqs"]), off
        if off == 1:
            mk = lambda k: [np.concatenate([rand(200 + k, 500), np.full(300, 9, np.uint8), rand(100, 501)])]
        elif off >= 253:
            mk = lambda k, off=off: far(off, k)
        else:
            mk = lambda k, off=off: [compose([(64, 40, off)], 510 + k, head=off + k)]
        out.append(_find(f"offset_{off}", "RAW1", mk, cond))

    # ---- a match that ends exactly at a block end (no trailing literals; the chunk goes on), and one with literals behind it
    def cond_trailing(want):
        def cond(T):
            b = T[0][0]
            assert b["matched"] and (b["trailing"] == 0) == want and len(T[0]) == 2, (b.get("matched"), b.get("trailing"))
        return cond
    out.append(_find("match_ends_at_block_end", "RAW5",
                     lambda k: [_pad_to(compose([(BLOCK - 3000 - 100, 100, 700 + k)], 600 + k, head=3000, tail=4001), 5)], cond_trailing(True)))
    out.append(_find("match_then_trailing_literals", "RAW5",
                     lambda k: [_pad_to(compose([(BLOCK - 3000 - 200, 100, 700 + k)], 610 + k, head=3000, tail=4101), 5)], cond_trailing(False)))

    # ---- a match of exactly MIN bytes is kept; one of MIN - 1 is dropped and the block is the literal-only writer's
    def cond_min(T):
        b = T[0][0]
        assert b["matched"] and [ml for _l, ml, _o in b["seqs"]] == [MIN], b.get("seqs")

    def cond_below(T):
        b = T[0][0]
        assert not b["matched"] and b["n_seq"] == 0 and b["kind"] == L.HUF, b
    sk = lambda n, seed: skewed(n, seed)
    out.append(_find("match_of_min", "RAW1", lambda k: [compose([(900, MIN, 400)], 700 + k, head=500 + k, tail=600, filler=sk)], cond_min))

    def below(k):   # the same payload with the copy one byte shorter: the model's parser sees MIN - 1, which is dropped
        return [compose([(900, MIN - 1, 400)], 700 + k, head=500 + k, tail=601, filler=sk)]
    out.append(_find("match_below_min", "RAW1", below, cond_below))

    # ---- literals sections of all four kinds
    def lit_kind(kind, streams, pred=lambda b: True):
        def cond(T):
            b = T[0][0]
            assert b["matched"] and b["lit_kind"] == kind and b["lit_streams"] == streams and pred(b), {k: v for k, v in b.items() if k != "seqs"}
        return cond
    # (Raw literals because there are fewer than 64 of them are out of reach: the first 64 positions of a sub-range find an empty
    # hash table, so a block with a match has 64 literals or more. Raw literals here are the ones Huffman does not shrink.)
    out.append(_find("literals_raw", "RAW1", lambda k: [compose([(100, 3000, 80)], 800 + k, head=100 + k, tail=40)], lit_kind(L.RAW, 0, lambda b: b["n_lit"] >= 64)))
    out.append(_find("literals_rle", "RAW1", lambda k: [np.full(SUB * 2 + k, 3, np.uint8)], lit_kind(L.RLE, 0, lambda b: b["n_lit"] >= 64)))
    out.append(_find("literals_one_stream", "RAW1", lambda k: [compose([(100, 3000, 50)], 810 + k, head=60 + k, tail=40, filler=lambda n, s: P.distinct(n, 3, s))],
                     lit_kind(L.HUF, 1)))
    out.append(_find("literals_four_streams", "RAW1", lambda k: [compose([(3000, 600, 900), (2000, 60, 100)], 820 + k, head=1000 + k, tail=500, filler=sk)],
                     lit_kind(L.HUF, 4)))

    # ---- 127 and 128 sequences: the sequence count in one byte and in two
    for count in (127, 128):
        s = [(70, 16, 66)] * (count + 12)

        def cond(T, count=count):
            assert T[0][0]["matched"] and T[0][0]["n_seq"] == count, T[0][0]["n_seq"]
        out.append(_find(f"sequences_{count}", "RAW1", lambda k, s=s: [compose(s[:len(s) - k % 13], 900 + k, head=300 + k, filler=sk)], cond))

    # ---- a sub-range whose match list is full (1024 matches of 4..7 bytes, dropped) in a block that also has a kept match
    def full_list(k):   # bytes of three values: a thousand matches of 4 bytes and a few more fill the list before the sub-range ends
        a = np.random.RandomState(1000 + k).randint(0, 3, SUB * 2).astype(np.uint8)
        return [_pad_to(np.concatenate([a, compose([(70, 16, 66), (50, 30, 80)], 1004 + k, head=100)]), 4)]

    def cond_full(T):   # (the parser stops a sub-range once its list has no room for a step's 16 matches)
        b = T[0][0]
        assert b["list_max"] > M.MAX_MATCHES - 16 and b["matched"], b["list_max"]
    out.append(_find("full_match_list", "RAW4", full_list, cond_full))

    # ---- as many kept matches as a block takes here: 16 sub-ranges of 12-byte copies at stride 16. Reached: thousands of
    # sequences per block (8116 of them: a two-byte count, four 2048-sequence rounds of the coder, a bit stream of 22 KiB, more
    # than one 16 KiB image); 16 x 1024 kept matches do not fit 16 x 8192 bytes.
    def dense(k):
        return [compose([(4, MIN, 16)] * ((BLOCK - 64) // 16 - 8), 1100 + k, head=64, tail=0)[:BLOCK - 4 * (k % 3)].copy()]

    def cond_dense(T):
        b = T[0][0]
        assert b["matched"] and b["n_seq"] > 3 * 2048 and b["seq_bits"] > 8 * 16384, (b["n_seq"], b.get("seq_bits"))
    out.append(_find("dense_block", "RAW4", dense, cond_dense))

    # ---- bit streams of a length = 0 and = 7 modulo 8
    for rem in (0, 7):
        def cond(T, rem=rem):
            b = T[0][0]
            assert b["matched"] and b["seq_bits"] % 8 == rem, b.get("seq_bits")
        out.append(_find(f"bits_mod8_{rem}", "RAW1",
                         lambda k: [compose([(70 + k, 33, 200), (17 + (k % 5), 35 + k, 300)], 1200, head=400, tail=100, filler=sk)], cond))

    # ---- (a block whose Compressed form is not smaller than the block is out of reach with MIN = 12: a kept match saves 12
    # bytes or more and costs less than 8 bytes of bits, and what a sequences section costs once -- a literals header of up to 3
    # bytes, count and modes, the 18 closing bits -- is 11 bytes at most with the first match's bits. loses_to_raw() below builds
    # such a block for a smaller MIN; tests/test_zstd_match_model.py holds the model's fallback with it.)

    # ---- two blocks in a chunk, one with matches and one without
    def cond_two(T):
        assert [b["matched"] for b in T[0]] == [True, False] and T[0][1]["kind"] == L.HUF, [b["matched"] for b in T[0]]
    def two(k):
        a = compose([(5000, 2000, 4000), (300, 50, 80)] * 10, 1400 + k, head=4100, tail=0, filler=sk)
        return [np.concatenate([a, skewed(BLOCK - a.size, 1401), skewed(32763, 1402)])]
    out.append(_find("two_blocks_one_matched", "RAW5", two, cond_two))

    # ---- a chunk of eight blocks: with sequences over Huffman, RLE and Raw literals, and without
    def eight(k):
        def full(a, seed):
            return np.concatenate([a, rand(BLOCK - a.size, seed)])
        return [_pad_to(np.concatenate([two(k)[0][:BLOCK], skewed(BLOCK, 1501), np.zeros(BLOCK, np.uint8), rand(BLOCK, 1502),
                                full(compose([(70, 16, 66), (900, 700, 80)] * 40, 1503 + k, head=100), 1504), skewed(BLOCK, 1505, 0.4),
                                np.full(BLOCK, 200, np.uint8), compose([(70, 16, 66)] * 300, 1506 + k, head=100, filler=sk)]), 32)]

    def cond_eight(T):
        got = [(b["matched"], b.get("lit_kind") if b["matched"] else b["kind"]) for b in T[0]]
        assert got == [(True, L.HUF), (False, L.HUF), (True, L.RLE), (False, L.RAW), (True, L.RAW), (False, L.HUF), (True, L.RLE), (True, L.HUF)], got
    out.append(_find("eight_blocks_mixed", "RAW32", eight, cond_eight))

    # ---- 1100 one-chunk clouds of 80 .. 107 bytes, most with one match: a second round of 1024 in every one-workgroup scan
    clouds = [compose([(30, 20 + k % 9, 25)], 2000 + k, head=25, tail=5 + k % 28, filler=sk) for k in range(1100)]

    def cond_many(T):
        assert len(T) == 1100 and sum(1 for c in T if c[0]["matched"]) > 1024 // 2 and all(len(c) == 1 for c in T)
    out.append(Case("1100_clouds", "RAW1", clouds, cond_many))
    return out


def loses_to_raw() -> np.ndarray:
    """one 5-byte match among incompressible bytes: with min_match = 4 the model keeps it, and the block is Raw all the same"""
    return compose([(500, 5, 80)], 1300, head=100, tail=300)


_grid = None
_models = {}


def grid():
    global _grid
    if _grid is None:
        _grid = _build()
    return _grid


def case(name: str) -> Case:
    return next(c for c in grid() if c.name == name)


def batches():
    """schema -> the cases that go into one encode call, in file order"""
    out = {}
    for c in grid():
        out.setdefault(c.schema, []).append(c)
    return out


def model(c: Case):
    """per cloud of the case: [(payload, the model's frame, trace of its blocks)] of its chunks (computed once and shared)"""
    if c.name not in _models:
        rows = []
        for cloud in c.clouds:
            row = []
            for p in chunk_payloads(c.schema, cloud):
                trace = []
                frame = M.frame_info(p, trace)
                row.append((p, np.frombuffer(frame, np.uint8), trace))
            rows.append(row)
        _models[c.name] = rows
    return _models[c.name]


def traces(c: Case):
    return [t for row in model(c) for _p, _f, t in row]
