"""cloudini_amd/csrc/crc32_combine.h against zlib.crc32: the header is compiled with sanitizers into a stand-alone program
(tests/cpp/crc32_combine_cli.cpp) that answers one query per line. No GPU.

crc32_combine(crc(A), crc(B), len(B)) == crc(A + B); crc32_shift(crc(A), n) == crc(A + n zeros) ^ crc(n zeros) (the shift is the
combination with a piece that contributes nothing but its length); three pieces combine in either grouping. Operands of zero
bytes only make the CRC a function of the length alone -- a wrong shift count shows there and nowhere else -- and operands that
begin with zero bytes tell a raw remainder (which does not see leading zeros) from a CRC (whose initial value does)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(0, 71)) + [4095, 4096, 4097, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1 << 24) + 3]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("crc32") / "crc32_combine_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "crc32_combine_cli.cpp"),
                    "-o", exe], check=True)

    def ask(queries):
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        got = [int(x) for x in r.stdout.split()]
        assert len(got) == len(queries)
        return got
    return ask


def _contents(n: int):
    rs = np.random.RandomState(n % 9973)
    rnd = rs.randint(0, 256, n).astype(np.uint8).tobytes()
    lead = bytes(min(n, 5)) + rnd[min(n, 5):]                 # begins with zero bytes
    return {"random": rnd, "zeros": bytes(n), "leading zeros": lead, "ff": b"\xff" * n}


def _splits(n: int):
    return sorted({0, n, n // 2, min(n, 1), max(0, n - 1), n // 3, min(n, 4096)})


def test_combine_and_shift_of_two_pieces(cli):
    queries, want = [], []
    for n in LENGTHS:
        for kind, data in _contents(n).items():
            for s in _splits(n):
                a, b = data[:s], data[s:]
                queries.append(f"C {zlib.crc32(a)} {zlib.crc32(b)} {len(b)}")
                want.append((zlib.crc32(data), ("combine", n, kind, s)))
                queries.append(f"S {zlib.crc32(a)} {len(b)}")
                want.append((zlib.crc32(a + bytes(len(b))) ^ zlib.crc32(bytes(len(b))), ("shift", n, kind, s)))
    got = cli(queries)
    bad = [w[1] for g, w in zip(got, want) if g != w[0]]
    assert not bad, bad[:10]


def test_three_way_splits_in_either_grouping(cli):
    cases = []
    for n in LENGTHS:
        for kind, data in _contents(n).items():
            cuts = sorted({(n // 3, 2 * n // 3), (0, n // 2), (n // 2, n), (min(1, n), max(min(1, n), n - 1)), (0, 0), (n, n)})
            for s, t in cuts:
                cases.append((data, s, t, (n, kind, s, t)))
    parts = [(zlib.crc32(d[:s]), zlib.crc32(d[s:t]), zlib.crc32(d[t:]), t - s, len(d) - t) for d, s, t, _ in cases]
    ab = cli([f"C {a} {b} {lb}" for a, b, _c, lb, _lc in parts])
    bc = cli([f"C {b} {c} {lc}" for _a, b, c, _lb, lc in parts])
    left = cli([f"C {x} {p[2]} {p[4]}" for x, p in zip(ab, parts)])
    right = cli([f"C {p[0]} {x} {p[3] + p[4]}" for x, p in zip(bc, parts)])
    for (d, _s, _t, what), le, ri in zip(cases, left, right):
        assert le == ri == zlib.crc32(d), what


def test_powers_multiplication_and_the_host_table(cli, tmp_path):
    one, x = 0x80000000, 0x40000000
    ns = [0, 1, 2, 3, 4, 5, 127, 128, 129, 32767, 32768, 32769, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 40) + 12345]
    powers = cli([f"P {n}" for n in ns])
    assert powers[0] == one and powers[1] == 0x00800000                     # x^8
    # x has order 2^32 - 1: exponents wrap there (8 n modulo it)
    order = (1 << 32) - 1
    ref = {}
    for n, p in zip(ns, powers):
        assert ref.setdefault((8 * n) % order, p) == p, n
    # x^(8 n) is what a CRC moves by over n zero bytes: crc(A + zeros) ^ crc(zeros) = crc(A) * x^(8 n)
    a = zlib.crc32(b"abc")
    got = cli([f"M {p} {a}" for p in powers[:12]])
    for n, g in zip(ns[:12], got):
        assert g == zlib.crc32(b"abc" + bytes(n)) ^ zlib.crc32(bytes(n)), n
    assert cli([f"M {one} 12345", f"M 12345 {one}", f"M {x} {one}", "M 0 4294967295"]) == [12345, 12345, x, 0]
    # the host's table CRC, continued from an earlier value
    data = np.random.RandomState(5).randint(0, 256, 100001).astype(np.uint8).tobytes()
    path = tmp_path / "bytes.bin"
    path.write_bytes(data)
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    assert cli([f"F {path}", f"F {path} {zlib.crc32(b'front')}", f"F {empty}", f"F {empty} 77"]) == \
        [zlib.crc32(data), zlib.crc32(data, zlib.crc32(b"front")), 0, 77]
