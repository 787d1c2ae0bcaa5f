"""cloudini_amd/csrc/host/zstd_stitch.hpp on frames of the device ZSTD writer's models (tests/zstd_lit_model.py,
tests/zstd_match_model.py): the header is compiled with sanitizers into a stand-alone program (tests/cpp/zstd_stitch_cli.cpp)
that cuts frames into block runs and assembles container frames from files. No GPU.

Every assembled frame is raw(h) + run + raw(4 bytes) + run + raw(t), the shape of a message in a container chunk (host bytes,
the chunks' frames with their [u32] prefixes between them, host bytes); libzstd must return the concatenation and
tests/zstd_seq_rules.py must accept the frame. Every frame form that is not the device writer's must be refused."""
import os
import subprocess

import numpy as np
import pytest

import zstd_decode_cases as K
import zstd_lit_model as L
import zstd_match_grid as G
import zstd_match_model as M
import zstd_payload_grid as P
import zstd_seq_rules as R
from test_zstd_lit_model import zstd_decompress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = (0, 1, 131071, 131072, 131073)
MAGIC = b"\x28\xb5\x2f\xfd"


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    folder = tmp_path_factory.mktemp("stitch")
    exe = str(folder / "zstd_stitch_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cloudini_amd", "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "zstd_stitch_cli.cpp"),
                    "-o", exe], check=True)
    count = [0]

    def put(data: bytes) -> str:
        count[0] += 1
        path = folder / f"f{count[0]}.bin"
        path.write_bytes(bytes(data))
        return str(path)

    def run(lines):
        script = folder / f"script{count[0]}.txt"
        count[0] += 1
        script.write_text("".join(x + "\n" for x in lines))
        r = subprocess.run([exe, str(script)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout[-2000:]
        return out
    return put, run


def _payloads():
    """(name, payload, the device writer's frame): literal-only frames of the payload grid, frames with sequences, a hand-made
    frame whose second block takes the first one's Huffman table"""
    out = []
    for name in ("skewed_63", "one_value", "skewed_255", "skewed_1024", "skewed_131104", "three_byte_last_block", "uniform",
                 "full_block_then_another_run", "eight_blocks_mixed"):
        c = P.case(name)
        payload, frame, trace = P.model(c)[0][0]
        out.append((name, payload.tobytes(), frame.tobytes()))
    kinds = {n: [(b["kind"], b["form"]) for b in P.model(P.case(n))[0][0][2]] for n in ("skewed_63", "one_value", "skewed_255", "skewed_1024")}
    assert kinds == {"skewed_63": [(L.RAW, None)], "one_value": [(L.RLE, None)], "skewed_255": [(L.HUF, 0)], "skewed_1024": [(L.HUF, 2)]}
    assert len(P.model(P.case("eight_blocks_mixed"))[0][0][2]) == 8
    out.append(("empty", b"", L.frame(b"")))
    sk = lambda n, seed: P.skewed(n, seed)
    for name, data in (("sequences_one_block", G.compose([(3000, 600, 900), (2000, 60, 100)], 820, head=1000, tail=500, filler=sk)),
                       ("sequences_raw_literals", G.compose([(100, 3000, 80)], 800, head=100, tail=40)),
                       ("sequences_two_blocks", np.concatenate([G.compose([(5000, 2000, 4000), (300, 50, 80)] * 10, 1400, head=4100, tail=0, filler=sk),
                                                                P.skewed(70000, 1401)]))):
        trace = []
        frame = M.frame_info(data, trace)
        assert any(b["matched"] for b in trace), name
        out.append((name, data.tobytes(), frame))
    name, frame, cap, payload = next(x for x in K.hand_frames() if x[0] == "treeless/11")
    assert frame[:5] == MAGIC + b"\xa0" and payload is not None
    out.append(("treeless_second_block", payload, frame))
    return out


@pytest.fixture(scope="module")
def payloads():
    return _payloads()


def test_runs_of_device_frames(cli, payloads):
    put, run = cli
    assert len(payloads) >= 12
    got = run([f"cut {put(f)}" for _n, _p, f in payloads])
    for (name, payload, frame), line in zip(payloads, got):
        kind, content, nbytes, last_header = line.split()
        assert kind == "run" and int(content) == len(payload), (name, line)
        if len(payload) == 0:
            assert int(nbytes) == 0 and frame[9:] == b"\x01\x00\x00", name       # the empty Raw block is dropped
            continue
        assert int(nbytes) == len(frame) - 9, name
        # the last header is where a walk by block headers ends, and it alone carries the last-block bit
        at, headers = 9, []
        while at < len(frame):
            h = int.from_bytes(frame[at:at + 3], "little")
            headers.append(at - 9)
            at += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
            assert (h & 1) == (at == len(frame)), name
        assert at == len(frame) and int(last_header) == headers[-1], (name, line)


def test_assembled_frames_decode_to_the_concatenation(cli, payloads):
    put, run = cli
    rs = np.random.RandomState(3)
    tail = rs.randint(0, 256, 37).astype(np.uint8).tobytes()
    heads = {h: put(rs.randint(0, 256, h).astype(np.uint8).tobytes()) for h in HEADS}
    tail_path = put(tail)
    lines, want = [], []
    for k, (name, payload, frame) in enumerate(payloads):
        other_name, other, other_frame = payloads[(k + 5) % len(payloads)]
        f1, f2 = put(frame), put(other_frame)
        prefix = len(other_frame).to_bytes(4, "little")
        pre = put(prefix)
        for h in HEADS:
            out = put(b"")
            lines.append(f"assemble {out} raw:{heads[h]} run:{f1} raw:{pre} run:{f2} raw:{tail_path}")
            want.append((name, other_name, h, out, open(heads[h], "rb").read() + payload + prefix + other + tail, len(payload), len(other)))
    got = run(lines)
    n_ok = 0
    for line, (name, other_name, h, out, whole, n_first, n_second) in zip(got, want):
        what = (name, other_name, h)
        frame = open(out, "rb").read()
        assert line.split() == ["frame", str(len(whole)), str(len(frame))], (what, line)
        assert frame[:5] == MAGIC + b"\xa0" and int.from_bytes(frame[5:9], "little") == len(whole), what
        assert zstd_decompress(np.frombuffer(frame, np.uint8), len(whole)) == whole, what
        verdict, blocks, sums = R.walk(frame, len(whole))
        assert verdict == R.OK, (what, verdict)
        if len(whole) < 20000:
            # (decode() also applies the device decoder's budget of block records, 2 + bytes / 64-ish for a short frame: a
            # frame of several small Raw blocks is then HOST, "decode it on the host", never CORRUPT)
            verdict, data = R.decode(frame, len(whole))
            assert verdict in (R.OK, R.HOST) and (verdict == R.HOST or data == whole), what
            n_ok += verdict == R.OK
        # Raw blocks of the host's bytes: the 4-byte prefix shares its block with the bytes in front of it wherever the run
        # between them is empty, and the head is cut at 128 KiB
        at, sizes, last_bits = 9, [], []
        while at < len(frame):
            hd = int.from_bytes(frame[at:at + 3], "little")
            sizes.append(((hd >> 1) & 3, hd >> 3))
            last_bits.append(hd & 1)
            at += 3 + (1 if (hd >> 1) & 3 == 1 else hd >> 3)
        assert at == len(frame) and last_bits == [0] * (len(sizes) - 1) + [1], what
        assert all(size <= 131072 for _k, size in sizes), what
        if h >= 131072:
            assert sizes[0] == (0, 131072), (what, sizes[:3])
        elif h and n_first:
            assert sizes[0] == (0, h), (what, sizes[:3])
        elif not n_first and n_second:                                 # nothing between the head and the prefix
            assert sizes[0] == (0, min(h + 4, 131072)), (what, sizes[:3])
        if name == "empty" and other_name == "empty":
            assert [k for k, _s in sizes] == [0] * len(sizes) and sum(s for _k, s in sizes) == len(whole), what
    assert n_ok >= 1                                                       # (the rules' full decode ran on some frame)


def test_an_assembly_of_nothing_is_an_empty_frame(cli):
    put, run = cli
    out = put(b"")
    empty = put(L.frame(b""))
    assert run([f"assemble {out} run:{empty} raw:{put(b'')}"]) == ["frame 0 12"]
    frame = open(out, "rb").read()
    assert frame == MAGIC + b"\xa0" + bytes(4) + b"\x01\x00\x00" and zstd_decompress(np.frombuffer(frame, np.uint8), 0) == b""


def test_other_frame_forms_are_refused(cli):
    put, run = cli
    a = P.skewed(700, 11)
    good = L.frame(a)
    blk = good[9:]
    two = L.frame(P.skewed(131072 + 500, 12))
    bad = {
        "window descriptor": K.frame_header(700, single=False, fcs_bytes=4) + blk,
        "no content size": K.frame_header(None, single=False, fcs_bytes=0) + blk,
        "1-byte content size": K.frame_header(200, single=True, fcs_bytes=1) + L.block(a[:200], True)[2],
        "2-byte content size": K.frame_header(700, single=True, fcs_bytes=2) + blk,
        "8-byte content size": K.frame_header(700, single=True, fcs_bytes=8) + blk,
        "checksum bit": good[:4] + b"\xa4" + good[5:] + bytes(4),
        "checksum behind the last block": good + bytes(4),
        "dictionary id": good[:4] + b"\xa1" + b"\x07" + good[5:],
        "reserved bit": good[:4] + b"\xa8" + good[5:],
        "skippable frame": b"\x50\x2a\x4d\x18" + (8).to_bytes(4, "little") + bytes(8),
        "magic": b"\x28\xb5\x2f\xfc" + good[4:],
        "no block": good[:9],
        "header only": good[:5],
        "empty": b"",
        "cut inside the last block": good[:-1],
        "cut inside a block header": two[:9 + 3 + (int.from_bytes(two[9:12], "little") >> 3) + 2],
        "no last block": two[:9 + 3 + (int.from_bytes(two[9:12], "little") >> 3)],
        "last bit on the first of two blocks": two[:9] + bytes([two[9] | 1]) + two[10:],
        "reserved block type": good[:9] + bytes([good[9] | 6]) + good[10:],
        "block size past the end": good[:9] + (int.from_bytes(good[9:12], "little") + (1 << 3)).to_bytes(3, "little") + good[12:],
        "block above 128 KiB": good[:5] + (131073).to_bytes(4, "little") + ((131073 << 3) | 1).to_bytes(3, "little") + bytes(131073),
        "blocks but content size 0": good[:5] + bytes(4) + blk,
        "content size but no block": good[:5] + (5).to_bytes(4, "little") + b"\x01\x00\x00",
    }
    names = list(bad)
    got = run([f"cut {put(bad[n])}" for n in names] + [f"cut {put(good)}"])
    assert got[-1].startswith("run 700 ")
    for name, line in zip(names, got):
        assert line.startswith("error zstd_stitch: "), (name, line)
    # and an assembly with such a piece fails as a whole
    assert run([f"assemble {put(b'')} raw:{put(b'abc')} run:{put(bad['checksum bit'])}"])[0].startswith("error ")
