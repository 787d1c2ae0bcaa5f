"""McapWriter's stitched chunks (include/cloudini_amd/mcap_io.hpp: addStitchedMessage, writeStitchedChunk) with frames of the
device ZSTD writer's models standing in for the device, and the readers' check of a non-zero uncompressed_crc. No GPU.

A script of ordinary and stitched messages goes through tests/cpp/mcap_stitch_cli.cpp; the file is read back by McapFile and
McapStream (tests/cpp/mcap_dump.cpp) and by the reader below, which decompresses every chunk with libzstd and checks what the
C++ readers check, from the published record layouts alone. A file written without the new calls must be the parent's, byte for
byte: tests/golden/mcap_rt_none.mcap is what tests/cpp/mcap_roundtrip.cpp wrote before this change."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import mcap_py
import zstd_lit_model as L
import zstd_match_grid as G
import zstd_match_model as M
import zstd_payload_grid as P
from test_zstd_lit_model import zstd_decompress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudini_amd", "lib")
CHUNK = 200000


def _build(folder, name):
    exe = str(folder / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "cloudini_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(LIB, "libcloudini_amd.so"),
                    os.path.join(LIB, "libcloudini_hip.so"), "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def _fnv(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return h


def read_checked(path):
    """-> (messages in file order, chunks [(crc, compression, records)], message index [(chunk number, channel, [(log, offset)])]).
    Every chunk is decompressed; a non-zero uncompressed_crc must be zlib.crc32 of its records."""
    b = open(path, "rb").read()
    assert b[:8] == mcap_py.MAGIC and b[-8:] == mcap_py.MAGIC
    msgs, chunks, index = [], [], []

    def records(buf, top):
        i = 0
        while i < len(buf):
            op, n = struct.unpack_from("<BQ", buf, i)
            body = buf[i + 9:i + 9 + n]
            assert len(body) == n
            i += 9 + n
            if op == mcap_py.MESSAGE:
                ch, seq, lt, pt = struct.unpack_from("<HIQQ", body, 0)
                msgs.append((ch, seq, lt, pt, body[22:]))
            elif op == mcap_py.CHUNK:
                assert top
                _t0, _t1, usize, crc = struct.unpack_from("<QQQI", body, 0)
                (cn,) = struct.unpack_from("<I", body, 28)
                comp = body[32:32 + cn].decode()
                (n2,) = struct.unpack_from("<Q", body, 32 + cn)
                packed = body[40 + cn:]
                assert len(packed) == n2
                recs = packed if comp == "" else zstd_decompress(packed, usize)
                assert comp in ("", "zstd") and len(recs) == usize
                if crc:
                    assert zlib.crc32(recs) == crc, "chunk crc mismatch"
                chunks.append((crc, comp, recs))
                records(recs, False)
            elif op == mcap_py.MESSAGE_INDEX:
                ch, nb = struct.unpack_from("<HI", body, 0)
                index.append((len(chunks) - 1, ch, [struct.unpack_from("<QQ", body, 6 + 16 * k) for k in range(nb // 16)]))
            elif op == mcap_py.DATA_END:
                return
    records(b[8:-8], True)
    return msgs, chunks, index


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    folder = tmp_path_factory.mktemp("mcap_stitched")
    return folder, _build(folder, "mcap_stitch_cli"), _build(folder, "mcap_dump")


def _frames():
    """payloads and the device writer's frames of them: Huffman one- and four-stream, two blocks, RLE, Raw, empty, with sequences"""
    sk = lambda n, seed: P.skewed(n, seed)
    payloads = [P.skewed(5000, 1), P.skewed(200, 2), P.skewed(131072 + 700, 3), np.full(3000, 9, np.uint8), P.skewed(40, 4),
                np.zeros(0, np.uint8), G.compose([(3000, 600, 900), (2000, 60, 100)], 820, head=1000, tail=500, filler=sk)]
    frames = [L.frame(p) for p in payloads[:-1]] + [M.frame(payloads[-1])]
    assert frames[-1] != L.frame(payloads[-1])                                      # (it has sequences)
    return [p.tobytes() for p in payloads], frames


def _write(tools, name, chunk=CHUNK):
    folder, cli, _dump = tools
    payloads, frames = _frames()
    n = [0]

    def put(data):
        n[0] += 1
        path = folder / f"{name}_{n[0]}.bin"
        path.write_bytes(bytes(data))
        return str(path)
    out = str(folder / f"{name}.mcap")
    lines = [f"open {out} {chunk}", "schema 1 sensor_msgs/msg/PointCloud2", "schema 2 x/msg/Y", "channel 3 1 /points", "channel 4 2 /other"]
    want = []
    rs = np.random.RandomState(8)
    seq = 0

    def ordinary():
        nonlocal seq
        d = rs.randint(0, 256, 50 + seq).astype(np.uint8).tobytes()
        lines.append(f"msg 4 {seq} {1000 + seq} {900 + seq} {put(d)}")
        want.append((4, seq, 1000 + seq, 900 + seq, d))
        seq += 1

    def stitched(ks):
        nonlocal seq
        head = rs.randint(0, 256, 60 + seq).astype(np.uint8).tobytes()
        tail = rs.randint(0, 256, 9).astype(np.uint8).tobytes()
        pieces, data = [f"raw:{put(head)}"], head
        for k in ks:                                                                # a stream of one chunk each, host bytes between
            one = struct.pack("<I", len(payloads[k])) + payloads[k]
            pieces += [f"stream:{zlib.crc32(one)}:{put(frames[k])}", f"raw:{put(b'|')}"]
            data += one + b"|"
        pieces.append(f"raw:{put(tail)}")
        data += tail
        lines.append(f"smsg 3 {seq} {1000 + seq} {900 + seq} " + " ".join(pieces))
        want.append((3, seq, 1000 + seq, 900 + seq, data))
        seq += 1

    def stitched_stream(ks):
        """the chunks of one cloud under ONE checksum, as the device takes it: [u32 size][payload] per chunk"""
        nonlocal seq
        head = rs.randint(0, 256, 33).astype(np.uint8).tobytes()
        stream = b"".join(struct.pack("<I", len(payloads[k])) + payloads[k] for k in ks)
        pieces = [f"raw:{put(head)}", f"stream:{zlib.crc32(stream)}:" + ",".join(put(frames[k]) for k in ks), f"raw:{put(b'tail')}"]
        lines.append(f"smsg 3 {seq} {1000 + seq} {900 + seq} " + " ".join(pieces))
        want.append((3, seq, 1000 + seq, 900 + seq, head + stream + b"tail"))
        seq += 1

    ordinary()
    ordinary()
    stitched([0])
    stitched([1, 3])
    ordinary()                                                                      # closes the stitched chunk
    stitched([2, 6])                                                                # 131072 + 700 + ...: the chunk is not yet full
    stitched([2])                                                                   # now it is: closed by the size rule
    stitched([5])                                                                   # an empty payload: host bytes only
    stitched([4, 5, 0])
    stitched_stream([0, 6, 1])
    stitched_stream([3])
    lines.append("channel 5 2 /late")                                               # a channel record in between
    stitched([6])
    lines.append("begin")
    stitched([0, 1])
    stitched([3])
    lines.append("end")                                                             # closed whatever its size
    stitched([1])
    ordinary()
    stitched([4])                                                                   # the file ends in an open stitched chunk
    lines.append("close")
    script = folder / f"{name}.txt"
    script.write_text("".join(x + "\n" for x in lines))
    r = subprocess.run([cli, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
    return out, want, payloads, frames


def test_every_reader_returns_the_messages_in_file_order(tools):
    _folder, _cli, dump = tools
    out, want, _p, _f = _write(tools, "order")
    msgs, chunks, index = read_checked(out)
    assert [(m[0], m[1], m[2], m[3]) for m in msgs] == [(m[0], m[1], m[2], m[3]) for m in want]
    assert [m[4] for m in msgs] == [m[4] for m in want]
    for mode in ([], ["stream"]):
        r = subprocess.run([dump, out] + mode, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        got = [l for l in r.stdout.splitlines() if l.startswith("message")]
        assert got == [f"message {c} {q} {lt} {pt} {len(d)} {_fnv(d)}" for c, q, lt, pt, d in want], mode
        assert [l for l in r.stdout.splitlines() if l.startswith("channel")] == ["channel 3 1 /points cdr 0", "channel 4 2 /other cdr 0", "channel 5 2 /late cdr 0"]
    # stitched chunks carry the CRC of their records (read_checked has compared it), ordinary chunks carry 0; a chunk holds
    # messages of one kind only, and every chunk is a "zstd" chunk
    kinds = []
    for crc, comp, recs in chunks:
        assert comp == "zstd"
        chans = set()
        i = 0
        while i < len(recs):
            op, n = struct.unpack_from("<BQ", recs, i)
            if op == mcap_py.MESSAGE:
                chans.add(struct.unpack_from("<H", recs, i + 9)[0])
            i += 9 + n
        assert chans <= {3} or chans <= {4}, chans
        if chans == {3}:
            assert crc == zlib.crc32(recs) != 0
        else:
            assert crc == 0
        kinds.append("s" if chans == {3} else "o")
    # the boundaries: ordinary | 2 stitched | ordinary (+ the late channel's record later) | the size rule | ... | the last one
    assert "".join(kinds) == "osossossos", kinds
    sizes = [len(recs) for crc, _c, recs in chunks if crc]
    assert sizes[1] >= CHUNK and all(s < CHUNK + 131072 + 2000 for s in sizes)     # closed as soon as CHUNK bytes are in
    # MessageIndex: one record per channel with messages behind every chunk; every offset points at that message's record
    seen = 0
    for k, ch, entries in index:
        recs = chunks[k][2]
        for lt, o in entries:
            assert recs[o] == mcap_py.MESSAGE
            got_ch, _seq, got_lt = struct.unpack_from("<HIQ", recs, o + 9)
            assert (got_ch, got_lt) == (ch, lt)
            seen += 1
    assert seen == len(want)


def test_a_flipped_bit_is_found(tools):
    folder, _cli, dump = tools
    out, want, payloads, frames = _write(tools, "flip")
    raw = open(out, "rb").read()

    def dumps(data, name):
        path = str(folder / name)
        open(path, "wb").write(data)
        return [subprocess.run([dump, path] + mode, capture_output=True, text=True, timeout=60) for mode in ([], ["stream"])]
    for r in dumps(raw, "same.mcap"):
        assert r.returncode == 0
    # one bit inside a device block (the blocks stand in the file as the device wrote them, but for the last-block bit)
    block = frames[0][9 + 3:]
    at = raw.find(block)
    assert at > 0
    for where in (at + len(block) // 2, at + 5, at + len(block) - 2):
        bad = bytearray(raw)
        bad[where] ^= 0x10
        for r in dumps(bytes(bad), "bit.mcap"):
            last = r.stdout.strip().splitlines()[-1]                               # (the stream reader has printed the header by then)
            assert r.returncode == 1 and last.startswith("error MCAP: ") and ("chunk crc mismatch" in last or "zstd" in last), r.stdout
        with pytest.raises(AssertionError):
            read_checked(str(folder / "bit.mcap"))
    # one bit of a stitched chunk's CRC field: the records are fine, the CRC is not theirs
    msgs, chunks, _ = read_checked(out)
    crc = next(c for c, _comp, _r in chunks if c)
    field = raw.find(struct.pack("<I", crc) + struct.pack("<I", 4) + b"zstd")
    assert field > 0
    bad = bytearray(raw)
    bad[field + 1] ^= 0x04
    for r in dumps(bytes(bad), "crc.mcap"):
        assert r.returncode == 1 and r.stdout.strip().splitlines()[-1] == "error MCAP: chunk crc mismatch", r.stdout
    # a CRC field of 0 is "not computed": the same records are then taken unchecked, as in every file written so far
    bad = bytearray(raw)
    bad[field:field + 4] = bytes(4)
    for r in dumps(bytes(bad), "zero.mcap"):
        assert r.returncode == 0


def test_a_damaged_frame_or_another_container_compression_aborts_the_file(tools, tmp_path):
    folder, cli, _dump = tools
    frame = L.frame(P.skewed(300, 5))
    f = tmp_path / "frame.bin"
    f.write_bytes(frame[:-1] + b"")                                                  # cut short: cut_device_frame refuses it
    script = tmp_path / "s.txt"
    script.write_text(f"open {tmp_path / 'x.mcap'} 1000\nschema 1 a\nchannel 3 1 /p\nsmsg 3 0 1 1 stream:5:{f}\nclose\n")
    r = subprocess.run([cli, str(script)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout.startswith("error zstd_stitch:"), r.stdout
    assert not os.path.exists(tmp_path / "x.mcap")                                   # an abandoned writer leaves nothing
    f.write_bytes(frame)
    for comp in ("none", "lz4"):
        script.write_text(f"open {tmp_path / 'y.mcap'} 1000 {comp}\nschema 1 a\nchannel 3 1 /p\nsmsg 3 0 1 1 stream:5:{f}\nclose\n")
        r = subprocess.run([cli, str(script)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout.startswith("error MCAP: a stitched chunk needs a zstd"), r.stdout
        assert not os.path.exists(tmp_path / "y.mcap")


def test_files_written_without_the_new_calls_are_the_parents(tmp_path):
    exe = _build(tmp_path, "mcap_roundtrip")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    golden = open(os.path.join(ROOT, "tests", "golden", "mcap_rt_none.mcap"), "rb").read()
    assert open(tmp_path / "rt_none.mcap", "rb").read() == golden
    # the compressed containers: the same records in the same chunks (what the compressors make of them is theirs), CRC 0
    msgs0, chunks0, index0 = read_checked(str(tmp_path / "rt_none.mcap"))
    msgs, chunks, index = read_checked(str(tmp_path / "rt_zstd.mcap"))
    assert msgs == msgs0 and index == index0
    assert [(c[0], c[2]) for c in chunks] == [(0, c[2]) for c in chunks0] and all(c[1] == "zstd" for c in chunks)
    assert all(c[0] == 0 for c in chunks0)


def test_the_tool_refuses_the_option_where_it_cannot_hold(tmp_path):
    """--mcap-device-zstd: not with --decode, a directory, another container compression or --device-zstd (exit status 2,
    before anything is opened)"""
    tool = os.path.join(LIB, "cloudini_batch_transcode")
    bag, out = str(tmp_path / "in.mcap"), str(tmp_path / "out.mcap")
    for args in ([bag, out, "--mcap-device-zstd", "--decode"], [str(tmp_path), str(tmp_path / "o"), "--mcap-device-zstd"],
                 [bag, out, "--mcap-device-zstd", "--mcap-compression", "lz4"], [bag, out, "--mcap-device-zstd", "--mcap-compression", "none"],
                 [bag, out, "--mcap-device-zstd", "--device-zstd"], [bag, out, "--device-zstd-matches"]):
        r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "needs" in r.stderr, (args, r.stderr)
    assert not os.path.exists(out)
