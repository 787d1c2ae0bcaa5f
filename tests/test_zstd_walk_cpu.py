"""cloudini_amd/csrc/zstd_decode_walk.h -- the header walk the device ZSTD decoder and the host mirror run -- compiled with
g++ -fsanitize=address,undefined into a stand-alone program (tests/cpp/zstd_walk_cli.cpp) and held against
tests/zstd_lit_rules.py: header-level verdict, block table and weights of every frame of tests/zstd_decode_cases.py. No GPU."""
import os
import struct
import subprocess

import zstd_decode_cases as K
import zstd_lit_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERDICT = {0: R.OK, 1: R.HOST, 2: R.CORRUPT}


def test_walk_header_matches_the_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "zstd_walk_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "zstd_walk_cli.cpp"),
                    "-o", exe], check=True)
    seed = int.from_bytes(os.urandom(4), "little") | 1
    cases = [(n, f, c) for n, f, c, _p in K.grid_frames() + K.libzstd_frames() + K.hand_frames()]
    cases += [(n, f, c - 1) for n, f, c, _p in K.grid_frames() if c]
    cases += K.damaged(seed)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _n, f, c in cases:
            fh.write(struct.pack("<II", len(f), c))
            fh.write(f)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())
    seen = {R.OK: 0, R.HOST: 0, R.CORRUPT: 0}
    for name, f, c in cases:
        v, n, total = map(int, next(lines).split())
        want_v, blocks, want_total = R.walk(f, c)
        assert (VERDICT[v], n, total) == (want_v, len(blocks), want_total), (seed, name)
        seen[want_v] += 1
        for i, b in enumerate(blocks):
            row = next(lines).split(" ")
            got = list(map(int, row[:10]))
            tree = b["tree"] if b["kind"] == R.HUF else R.NO_TREE
            want = [b["kind"], b["src"], b["size"], b["out"], b["regen"], b["streams"], tree, b["desc"], b.get("log", 0), len(b.get("weights", []))]
            assert got == want, (seed, name, i)
            assert row[10] == bytes(b.get("weights", [])).hex(), (seed, name, i)
    assert next(lines, None) is None and min(seen.values()) > 100, seen
