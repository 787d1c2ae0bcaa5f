"""zd_walk_seq of cloudini_amd/csrc/zstd_decode_walk.h -- the header walk of the device ZSTD decoder with the sequences switch
on -- compiled with g++ -fsanitize=address,undefined into a stand-alone program (tests/cpp/zstd_seq_walk_cli.cpp) and held
against tests/zstd_seq_rules.py: verdict, records, sequence records, sums and the decode tables of every FSE description, of
every frame of tests/zstd_seq_cases.py and of the frames of tests/zstd_decode_cases.py. No GPU; nothing is preloaded."""
import os
import struct
import subprocess

import zstd_decode_cases as K
import zstd_seq_cases as Q
import zstd_seq_rules as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERDICT = {0: S.OK, 1: S.HOST, 2: S.CORRUPT}


def _table_sum(seq):
    total = 0
    for t in range(3):
        if seq["modes"][t] == S.FSE:
            norm, log = seq["norm"][t]
            for sym, nb, base in S.fse_table(norm, log):
                total = (total * 31 + (sym | (nb << 8) | ((base & 0xFFFF) << 16))) & 0xFFFFFFFF
    return total


def test_seq_walk_matches_the_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "zstd_seq_walk_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "zstd_seq_walk_cli.cpp"),
                    "-o", exe], check=True)
    cases = [(n, f, c) for n, f, c, _p in Q.grid_frames() + Q.libzstd_frames() + K.grid_frames() + K.libzstd_frames() + K.hand_frames()]
    cases += [c for i in range(len(Q.damage_bases())) for c in Q.damaged_base(i)] + Q.random_damage()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _n, f, c in cases:
            fh.write(struct.pack("<II", len(f), c))
            fh.write(f)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())
    seen = {S.OK: 0, S.HOST: 0, S.CORRUPT: 0}
    seq_frames = 0
    for name, f, c in cases:
        v, n, total, has_seq, seqs, lits, n_all, n_regen = map(int, next(lines).split())
        _cv, _cb, csums = S.walk(f, c, all_blocks=None, read_trees=False)
        want_v, blocks, sums = S.walk(f, c, all_blocks=csums["has_seq"])
        assert (VERDICT[v], n) == (want_v, len(blocks)), name
        assert (has_seq, seqs, lits, n_all, n_regen) == (int(sums["has_seq"]), sums["seqs"], sums["lits"], sums["n_all"], sums["n_regen"]), name
        if not sums["has_seq"]:
            assert total == sums["total"], name
        seen[want_v] += 1
        seq_frames += want_v == S.OK and sums["has_seq"]
        for i, b in enumerate(blocks):
            got = list(map(int, next(lines).split()))
            tree = b["tree"] if b["kind"] == S.HUF else S.NO_TREE
            want = [b["kind"], b["src"], b["size"], b["out"], b["regen"], b["streams"], tree, b["desc"], b.get("log", 0), len(b.get("weights", [])),
                    int(csums["has_seq"])]
            assert got[:11] == want, (name, i)
            q = b["seq"]
            if q is None:
                assert got[11] == 0, (name, i)
                continue
            modes = q["modes"][0] | (q["modes"][1] << 2) | (q["modes"][2] << 4) | (q["form"] << 8)
            tabs = [q["tab"][t][0] if q["tab"][t][1] else 0 for t in range(3)]
            assert got[11:] == [q["nb"], modes] + tabs + q["rep"] + list(q["bits"]) + [q["first"], _table_sum(q)], (name, i)
    assert next(lines, None) is None and min(seen.values()) > 100 and seq_frames > 100, (seen, seq_frames)
