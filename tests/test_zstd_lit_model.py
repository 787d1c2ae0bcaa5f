"""The model of the device ZSTD writer (tests/zstd_lit_model.py) against libzstd: every frame of the payload grid
(tests/zstd_payload_grid.py) decodes to its payload, every case is what it was built for, no frame exceeds ZSTD_COMPRESSBOUND;
and the frames' sizes against ZSTD_compress(level 1) on the stage-1 payloads of the two golden sample slices. No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import sweep_model as S
import zstd_lit_model as M
import zstd_payload_grid as G
from cloudini_amd import api

ZSTD_SO = "libzstd.so.1"
_z = None


def zstd():
    global _z
    if _z is None:
        _z = C.CDLL(ZSTD_SO)
        _z.ZSTD_decompress.restype = C.c_size_t
        _z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        _z.ZSTD_compress.restype = C.c_size_t
        _z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
        _z.ZSTD_isError.argtypes = [C.c_size_t]
        _z.ZSTD_getErrorName.restype = C.c_char_p
        _z.ZSTD_getErrorName.argtypes = [C.c_size_t]
        _z.ZSTD_compressBound.restype = C.c_size_t
        _z.ZSTD_compressBound.argtypes = [C.c_size_t]
    return _z


def zstd_decompress(frame, size: int) -> bytes:
    """the frame through ZSTD_decompress with room for exactly `size` bytes"""
    z = zstd()
    frame = bytes(frame)
    out = C.create_string_buffer(max(1, size))
    r = z.ZSTD_decompress(out, size, frame, len(frame))
    assert not z.ZSTD_isError(r), z.ZSTD_getErrorName(r).decode()
    return out.raw[:r]


def zstd_level1_size(payload: bytes) -> int:
    z = zstd()
    cap = z.ZSTD_compressBound(len(payload))
    out = C.create_string_buffer(max(1, cap))
    r = z.ZSTD_compress(out, cap, payload, len(payload), 1)
    assert not z.ZSTD_isError(r)
    return int(r)


@pytest.mark.parametrize("name", [c.name for c in G.grid()])
def test_grid_frames_decode_through_libzstd(name):
    c = G.case(name)
    for row in G.model(c):
        for payload, frame, trace in row:
            assert zstd_decompress(frame, payload.size) == payload.tobytes()
            assert frame.size <= M.bound(payload.size) == zstd().ZSTD_compressBound(payload.size)
            assert len(trace) == max(1, (payload.size + M.BLOCK - 1) // M.BLOCK)
            assert M.frame(payload) == frame.tobytes()                          # (deterministic)
    c.cond(G.traces(c))


def test_grid_covers_every_kind_and_form():
    seen = set()
    for c in G.grid():
        for t in G.traces(c):
            for b in t:
                seen.add((b["kind"], b["form"]))
                seen.add(b.get("description"))
                seen.add(("weights odd", b.get("weights", 0) % 2))
                seen.add(("clamped", b.get("clamped")))
                seen.add(("why", b.get("why_raw")))
    for want in [(M.RAW, None), (M.RLE, None), (M.HUF, 0), (M.HUF, 1), (M.HUF, 2), (M.HUF, 3), "direct", "fse", ("weights odd", 0),
                 ("weights odd", 1), ("clamped", True), ("clamped", False), ("why", "short"), ("why", "not smaller")]:
        assert want in seen, want
    assert len(G.batches()) == 4 and all(c.name in [x.name for x in G.grid()] for c in map(G.case, G.ALIGNMENT_CASES))


def test_empty_payload_and_mixed_code_lengths():
    assert M.frame(b"") == bytes.fromhex("28b52ffda0" "00000000" "010000") and zstd_decompress(M.frame(b""), 0) == b""
    # 256 symbols whose code lengths change from one symbol to the next: the longest tree descriptions this writer makes
    rs = np.random.RandomState(3)
    counts = np.where(np.arange(256) % 2 == 0, 2, 1) * np.array([1, 1, 2, 4, 8, 16, 32, 64] * 32)
    data = rs.permutation(np.repeat(np.arange(256, dtype=np.uint8), counts))
    frame, kinds = M.frame_info(data)
    assert zstd_decompress(frame, data.size) == data.tobytes()
    assert kinds == [(M.HUF, 2)]


def test_code_lengths_are_complete_and_clamped():
    rs = np.random.RandomState(5)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    shapes = [np.array(fib[:k]) for k in (2, 3, 12, 13, 24, 40)] + [rs.randint(1, 1000, k) for k in (2, 5, 100, 256)] + \
             [np.ones(k, np.int64) for k in (2, 3, 255, 256)] + [np.array([1] * 200 + [10 ** 6] * 3)]
    for sh in shapes:
        counts = np.zeros(256, np.int64)
        counts[rs.permutation(256)[:len(sh)]] = sh
        lens = M.code_lengths(counts)
        assert ((lens > 0) == (counts > 0)).all() and lens.max() <= M.MAX_LEN
        assert sum(1 << (M.MAX_LEN - int(l)) for l in lens if l) == 1 << M.MAX_LEN
        order = np.argsort(counts[counts > 0], kind="stable")
        assert (np.diff(lens[counts > 0][order]) <= 0).all()                    # a rarer symbol never has the shorter code


# ---- sizes against libzstd level 1 -------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v1.npz")
# Measured (this test prints the table): literal-only frames over ZSTD_compress(level 1), per chunk payload of the
# slice, over the five rungs of the default ladder. lidar.pcd is XYZI float32, all tokens: the frames are within a percent of
# libzstd's. The assertion is the measured range widened by 0.02. dds_message.bin carries a ring and a lossless float64 stamp
# whose bytes repeat: ZSTD's matches halve them and a writer without matches cannot; recorded, not bounded.
#   sample_lidar_pcd_8000    rungs 0-4: 34641/34641, 40477/40470, 37056/36753, 28997/28997, 21898/21905 -> 0.9997 .. 1.0082
#   sample_dds_message_6000  rungs 0-4: 29408/15374, 34785/18251, 32033/16900, 25176/12796, 21066/9986  -> 1.895 .. 2.110
LIDAR_RATIOS = (0.9997, 1.0082)
SLICES = ["sample_lidar_pcd_8000", "sample_dds_message_6000"]


def _golden(name):
    z = np.load(GOLDEN)
    info = api.parse_yaml_info(z[name + "/yaml"].tobytes().decode(), int(z[name + "/version"][0]))
    info.use_threads = False
    return info, z[name + "/input"]


def size_rows(oracle):
    rows = []
    for name in SLICES:
        info, data = _golden(name)
        kinds = S.field_kinds(info)
        ladders = S.default_ladders(info)
        for c in range(ladders.shape[1]):
            rung = info.copy()
            for f, kind in enumerate(kinds):
                if kind != S.NONE:
                    rung.fields[f].resolution = float(ladders[f, c])
            stream = oracle.encode_stage1(rung, data)
            stage1 = ours = theirs = 0
            o = 0
            while o < stream.size:
                n = int.from_bytes(stream[o:o + 4].tobytes(), "little")
                payload = stream[o + 4:o + 4 + n]
                frame = M.frame(payload)
                assert zstd_decompress(frame, n) == payload.tobytes()
                stage1, ours, theirs = stage1 + n, ours + len(frame), theirs + zstd_level1_size(payload.tobytes())
                o += 4 + n
            rows.append((name, c, stage1, ours, theirs, ours / theirs))
    return rows


def test_frame_sizes_against_libzstd_level_1(oracle):
    rows = size_rows(oracle)
    for name, c, stage1, ours, theirs, ratio in rows:
        print(f"{name} rung {c}: stage-1 {stage1} B, literal-only frames {ours} B, libzstd level 1 {theirs} B, ratio {ratio:.4f}")
    for name, c, stage1, ours, theirs, ratio in rows:
        if name == SLICES[0]:
            assert LIDAR_RATIOS[0] - 0.02 <= ratio <= LIDAR_RATIOS[1] + 0.02, (name, c, ratio)
