"""The memory the stage-2 kernels and the viz and decode calls run in: every workspace is laid out by one carve function
(cloudini_amd/csrc/workspace_carve.h), whose run over NULL is the size the call allocates. No GPU:
  * stage2_launch.h, status_block.h and encode_workspace.h each build by themselves with a plain compiler;
  * the sizes against the closed forms the code had before the carve (restated here from stage1_launch.h and hip_abi.hip of
    that time, with the record sizes the shim exports): the encoder workspaces are as large as they were to the byte, the
    others at least as large and less than one alignment step larger; the viz tables (encode_workspace.h) as large as they
    were to the byte;
  * hip_abi.hip addresses the decode counters and the size of the status block (status_block.h) by name;
  * tests/cpp/workspace_cli.cpp under sanitizers: every array written over its documented length inside an allocation of
    exactly that size -- no overrun, no overlap, the documented alignment, the slack behind the last array;
  * the carver itself."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

from cloudini_amd import build as _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cloudini_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_build.HIPCC))), "include")
GXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]

CHUNKS = (0, 1, 7, 993)
LZ4_GRID = list(itertools.product((0, 1, 5, 1025), CHUNKS))                                    # max_subs, chunks
ZSTD_SEQ_GRID = list(itertools.product((0, 1, 5, 1025), (0, 1, 9), CHUNKS))                     # max_subs, max_blocks, chunks
ZSTD_GRID = list(itertools.product((0, 1, 9, 257), CHUNKS))                                     # max_blocks, chunks
ZSTD_DECODE_GRID = list(itertools.product((0, 1, 100, 4097), CHUNKS, (0, 1, 2, 3, 12345, 1000003), (0, 1)))  # max_recs, frames, output bytes, sequences
ABI_GRID = list(itertools.product((1, 8, 9, 300), (0, 1, 2, 1000)))                             # n_clouds, n_chunks
VIZ_GRID = list(itertools.product((1, 8, 300), (0, 1, 1000)))                                   # n_clouds, viz blocks
PROGRAM_CASES = (len(LZ4_GRID) + len(ZSTD_SEQ_GRID) + len(ZSTD_GRID) + len(ZSTD_DECODE_GRID) + len(ABI_GRID) + 4 * (2 + 1 + 1 + 4) +
                 len(VIZ_GRID))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("carve") / "libcarve.so")
    subprocess.run(GXX + ["-O1", "-fPIC", "-shared", os.path.join(ROOT, "tests", "workspace_shim.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    for name, args in (("ws_lz4", [u64, u32]), ("ws_zstd_seq", [u64, u64, u32]), ("ws_zstd", [u64, u32]),
                       ("ws_zstd_decode", [u32, u32, C.c_int, u64]), ("ws_dec_meta", [u32, u32]), ("ws_dec_secs", [u32, u32]),
                       ("ws_span_tables", [u32]), ("ws_s2_gather", [u32]), ("ws_zstd_chunks", [u32, u32, C.c_int, u64, C.POINTER(u64)]),
                       ("ws_carver", [u64, C.POINTER(u64), u32, C.POINTER(u64)]), ("ws_carver_natural", [C.POINTER(u64)]),
                       ("ws_viz_tables", [u32, u32, C.POINTER(u64), C.POINTER(u64)])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = u64
    L.ws_sizeof.restype = u32
    return L


@pytest.fixture(scope="module")
def sizes(shim):
    names = ("ZdBlock", "ZdFse", "ZdSeqBlock", "ZdSeqSums", "ZsBlock", "ZsSeqPlan", "ZsSeqInfo", "DecChunk", "LzMatch",
             "VizCloud", "VizBlock")
    s = {n: shim.ws_sizeof(k) for k, n in enumerate(names)}
    assert all(s.values()) and s["LzMatch"] == 8      # (the old ZstdSeqLaunch formula wrote LzMatch as 8u)
    return s


def up(v, a):
    return (v + a - 1) // a * a


# ---- the closed forms of the sizes as they stood in front of the carve ------------------------------------------------------

def old_lz4(max_subs, n_chunks):
    return (7 * max_subs + n_chunks + (n_chunks + 1)) * 4


def old_zstd_seq(s, m, max_blocks, n_chunks):
    return (up(m * 8192, 64) + up(m * 1024 * 8, 64) * 2 + up(m * 1024 * 4, 64) + up(m * 4, 64) * 5 + up((n_chunks + 1) * 4, 64) +
            up(max_blocks * s["ZsSeqPlan"], 64) + up(max_blocks * s["ZsSeqInfo"], 64))


def old_zstd(s, max_blocks, n_chunks):
    codes = up(max_blocks * s["ZsBlock"], 64)
    descs = codes + max_blocks * 256 * 4
    block_dst = up(descs + max_blocks * 128, 64)
    blk_first = block_dst + (max_blocks + 1) * 8
    chunk_state = blk_first + (n_chunks + 1) * 4
    return chunk_state + n_chunks * 4


def old_zstd_decode(s, max_recs, n_frames, seq_on, out_bytes):
    seq = max_recs * s["ZdSeqBlock"] + n_frames * (s["ZdSeqSums"] + 8) + (out_bytes // 3 + 1) * 8 + out_bytes + 1024
    return up(max_recs * s["ZdBlock"], 256) + max_recs * 256 + 1024 * s["ZdFse"] + n_frames * 16 + 256 + (seq if seq_on else 0)


def old_dec_meta(s, n_clouds, n_chunks):
    table_bytes = (n_clouds + 1) * 20
    return up(table_bytes, 64) + up(max(1, n_chunks) * s["DecChunk"], 64) + max(1, n_chunks) * 18 + 64


def old_dec_secs(s, n_adaptive, n_chunks):
    return n_adaptive * n_chunks * s["DecChunk"] + n_chunks * 8 + 256


# (hip_abi.hip: clouds_b + blocks_b + kept_b of the viz filter)
def old_viz_tables(s, n_clouds, n_blocks):
    return up(n_clouds * s["VizCloud"], 64) + up(n_blocks * s["VizBlock"], 64) + (n_clouds + 1) * 8


# ---- tests -----------------------------------------------------------------------------------------------------------------

def _builds_alone(tmp_path, header):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\n' % header)
    subprocess.run(GXX + ["-fsyntax-only", str(src)], check=True)


def test_header_builds_alone(tmp_path):
    _builds_alone(tmp_path, "stage2_launch.h")


@pytest.mark.parametrize("header", ["status_block.h", "encode_workspace.h"])
def test_the_status_block_and_encode_workspace_headers_build_alone(tmp_path, header):
    _builds_alone(tmp_path, header)


def test_encoder_workspaces_are_as_large_as_they_were(shim, sizes):
    for m, nc in LZ4_GRID:
        assert shim.ws_lz4(m, nc) == old_lz4(m, nc), (m, nc)
    for m, mb, nc in ZSTD_SEQ_GRID:
        assert shim.ws_zstd_seq(m, mb, nc) == old_zstd_seq(sizes, m, mb, nc), (m, mb, nc)
    for mb, nc in ZSTD_GRID:
        assert shim.ws_zstd(mb, nc) == old_zstd(sizes, mb, nc), (mb, nc)


def test_zstd_decode_workspace_is_no_smaller_and_less_than_1024_bytes_larger(shim, sizes):
    for mr, nf, ob, seq in ZSTD_DECODE_GRID:
        grown = shim.ws_zstd_decode(mr, nf, seq, ob) - old_zstd_decode(sizes, mr, nf, seq, ob)
        assert 0 <= grown < 1024, (mr, nf, ob, seq, grown)


def test_abi_workspaces_are_no_smaller_and_less_than_256_bytes_larger(shim, sizes):
    for n_clouds, nc in ABI_GRID:
        grown = shim.ws_dec_meta(n_clouds, nc) - old_dec_meta(sizes, n_clouds, nc)
        assert 0 <= grown < 256, ("d_dec_meta", n_clouds, nc, grown)
    for nc in (0, 1, 2, 1000):
        for na in (1, 4):
            grown = shim.ws_dec_secs(na, nc) - old_dec_secs(sizes, na, nc)
            assert 0 <= grown < 256, ("d_dec_secs", na, nc, grown)
        assert shim.ws_span_tables(nc) == (nc + 1) * 16 + nc * 4       # d_lzd_tables
        assert shim.ws_s2_gather(nc) == nc * 8                         # d_s2_gather


def test_viz_tables_are_as_large_as_they_were(shim, sizes):
    at = (C.c_uint64 * 3)()
    dev = C.c_uint64()
    for n_clouds, nb in VIZ_GRID:                                                 # h_viz, and its prefix d_viz_tables
        assert shim.ws_viz_tables(n_clouds, nb, at, C.byref(dev)) == old_viz_tables(sizes, n_clouds, nb), (n_clouds, nb)
        clouds_b, blocks_b = up(n_clouds * sizes["VizCloud"], 64), up(nb * sizes["VizBlock"], 64)
        assert list(at) == [0, clouds_b, clouds_b + blocks_b] and dev.value == clouds_b + blocks_b


def test_hip_abi_addresses_the_decode_counters_and_the_block_s_size_by_name():
    """(The encode call still reaches k_finish's ticket and the contiguity flag as d_status.p + 40 and + 42.)"""
    text = open(os.path.join(CSRC, "hip_abi.hip")).read()
    assert not re.search(r"d_status\.p\s*\+\s*8\b", text) and not re.search(r"\bhs\[\s*\d", text)
    assert not re.search(r"d_status\.ensure\(\d", text) and not re.search(r"Memset\w*\(c->d_status\.p, 0, \d", text)  # (its size)


def test_zstd_workspace_of_a_decode_call_keeps_the_chunk_sizes_behind_the_decoder_s(shim, sizes):
    """d_zsd_ws of cldn_hip_decode_zstd was [ZstdDecodeLaunch::workspace_bytes rounded up to 256 | u32 per chunk], and is: the
    split adds nothing of its own. Against the old size of the whole it is what the decoder's part grew by (less than 1024,
    above), moved to the next multiple of 256 (less than 256 more)."""
    for nc in (0, 1, 2, 1000):
        for mr in (1, 100):
            for seq in (0, 1):
                slot_bytes = nc * 12352
                at = C.c_uint64()
                total = shim.ws_zstd_chunks(mr, nc, seq, slot_bytes, C.byref(at))
                inner = shim.ws_zstd_decode(mr, nc, seq, slot_bytes)
                assert at.value == up(inner, 256) and total == at.value + nc * 4
                grown = total - (up(old_zstd_decode(sizes, mr, nc, seq, slot_bytes), 256) + nc * 4)
                assert 0 <= grown < 1024 + 256, (mr, nc, seq, grown)


def test_every_array_fits_its_workspace_under_sanitizers(tmp_path):
    exe = str(tmp_path / "workspace_cli")
    subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          os.path.join(ROOT, "tests", "cpp", "workspace_cli.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.splitlines()[-1] == "ok %d" % PROGRAM_CASES


def _model(steps):
    """The carver restated: the offsets take returns (None for a pad) and the bytes reached."""
    off, at = 0, []
    for elem, count, align in steps:
        if elem == 0:
            off += count
            at.append(None)
        else:
            off = up(off, align)
            at.append(off)
            off += elem * count
    return at, off


CARVER_STEPS = [
    [(1, 0, 1)],                                                      # nothing at all
    [(0, 0, 1)],                                                      # pad(0)
    [(1, 3, 1), (4, 0, 256), (1, 1, 1)],                              # a count of 0 still rounds the offset up
    [(1, 1, 1), (8, 2, 8), (0, 0, 1), (1, 5, 1), (4, 3, 4), (0, 7, 1), (2, 1, 2)],
    [(4, 5, 256), (4, 5, 256), (1, 255, 1), (8, 1, 256), (0, 1024, 1)],
    [(1, 256, 1), (4, 1, 256), (1, 1, 256)],                          # an offset that is aligned already does not move
]


@pytest.mark.parametrize("steps", CARVER_STEPS)
def test_the_carver(shim, steps):
    want_at, want_bytes = _model(steps)
    flat = (C.c_uint64 * (3 * len(steps)))(*[x for s in steps for x in s])
    for base in (0, 0x7000_0000_1000):                                # NULL: a sizing pass; else an address nobody touches
        at = (C.c_uint64 * len(steps))()
        assert shim.ws_carver(base, flat, len(steps), at) == want_bytes
        for got, want in zip(at, want_at):
            assert got == (0 if want is None or base == 0 else base + want)


def test_the_carver_aligns_a_type_naturally_by_default(shim):
    at = (C.c_uint64 * 3)()
    assert shim.ws_carver_natural(at) == 24 and list(at) == [2, 16, 24]
