"""The model of the device ZSTD writer with matches (tests/zstd_match_model.py) on the CPU: every frame of the grid
(tests/zstd_match_grid.py) decodes through libzstd and through tests/zstd_seq_rules.py, every case is what it was built for, no
frame exceeds the bound; the sizes on the two golden slices for every candidate of kZsMinMatch, and the rule that picks it; and
cloudini_amd/csrc/zstd_seq_code.h, compiled with sanitizers into a stand-alone program, against the model's codes and states."""
import os
import subprocess

import numpy as np
import pytest

import sweep_model as S
import zstd_lit_model as L
import zstd_match_grid as G
import zstd_match_model as M
import zstd_seq_rules as R
from test_zstd_lit_model import SLICES, _golden, zstd, zstd_decompress, zstd_level1_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [c.name for c in G.grid()])
def test_grid_frames_decode_and_reach_their_condition(name):
    c = G.case(name)
    c.cond(G.traces(c))                                                          # before anything else
    for row in G.model(c):
        for payload, frame, trace in row:
            assert zstd_decompress(frame, payload.size) == payload.tobytes()
            verdict, got = R.decode(frame.tobytes(), payload.size)
            assert verdict == R.OK and got == payload.tobytes()
            assert frame.size <= M.L.bound(payload.size) == zstd().ZSTD_compressBound(payload.size)
            assert frame.size <= payload.size + 9 + 3 * len(trace)
            assert len(trace) == max(1, (payload.size + M.BLOCK - 1) // M.BLOCK)
            assert M.frame_info(payload) == frame.tobytes()                        # (deterministic)


def test_a_frame_without_kept_matches_is_the_literal_only_frame():
    for c in map(G.case, ["match_below_min"]):
        for row in G.model(c):
            for payload, frame, trace in row:
                assert frame.tobytes() == L.frame(payload)
    import zstd_payload_grid as P
    for name in ("skewed_16384", "uniform", "one_value_63", "three_byte_last_block"):
        for cloud in P.case(name).clouds:
            for p in P.chunk_payloads(P.case(name).schema, cloud):
                t = []
                f = M.frame_info(p, t)
                if all(not b["matched"] for b in t):
                    assert f == L.frame(p), name
                assert zstd_decompress(f, p.size) == p.tobytes()


def test_grid_covers_what_it_lists():
    seen = set()
    ll_codes, ml_codes, of_codes = set(), set(), set()
    for c in G.grid():
        for t in G.traces(c):
            for b in t:
                if not b["matched"]:
                    seen.add(("unmatched", b["kind"]))
                    continue
                seen.add(("lit", b["lit_kind"], b["lit_streams"]))
                seen.add(("count bytes", 1 if b["n_seq"] < 128 else 2))
                seen.add(("trailing", b["trailing"] == 0))
                seen.add(("bits mod 8", b["seq_bits"] % 8))
                seen.add(("image tiles", min(2, (b["seq_bits"] + 8 * 15) // (8 * 16384) + 1)))
                seen.add(("full list", b["list_max"] > M.MAX_MATCHES - 16))
                for ll, ml, off in b["seqs"]:
                    ll_codes.add(M.ll_code(ll))
                    ml_codes.add(M.ml_code(ml - 3))
                    of_codes.add(M.highbit(off + 3))
    for want in [("lit", L.RAW, 0), ("lit", L.RLE, 0), ("lit", L.HUF, 1), ("lit", L.HUF, 4), ("count bytes", 1), ("count bytes", 2),
                 ("trailing", True), ("trailing", False), ("bits mod 8", 0), ("bits mod 8", 7), ("image tiles", 2), ("full list", True),
                 ("unmatched", L.HUF), ("unmatched", L.RAW)]:
        assert want in seen, want
    assert ll_codes >= set(range(15, 36)), sorted(set(range(36)) - ll_codes)       # literal lengths 15 .. 65536 and beyond
    assert ml_codes >= set(range(31, 49)) | {M.MIN_MATCH - 3}, sorted(set(range(31, 49)) - ml_codes)   # match lengths 12, 34 .. 4098, the longest
    assert of_codes == set(range(2, 13)), of_codes
    assert all(c.name in [x.name for x in G.grid()] for c in map(G.case, G.ALIGNMENT_CASES)) and len(G.batches()) == 4


def test_raw_fallback_of_the_model():
    """With kZsMinMatch = 12 a block with sequences is always smaller than the block (zstd_match_grid._build says why); the
    fallback is held on the model with a smaller threshold."""
    p = G.loses_to_raw()
    t = []
    f = M.frame_info(p, t, min_match=4)
    assert t[0]["why_raw"] == "matches do not pay" and t[0]["kind"] == L.RAW and len(f) == p.size + 9 + 3
    assert zstd_decompress(f, p.size) == p.tobytes()
    t = []
    f = M.frame_info(p, t)
    assert not t[0]["matched"] and f == L.frame(p)                                 # (5 bytes: dropped at 12)


def test_sequence_count_forms_and_code_tables():
    assert M.MAX_SEQ == 16384 < 0x7F00
    for ll in range(0, 131072):
        c = M.ll_code(ll)
        assert M.LL_BASE[c] <= ll < (M.LL_BASE[c + 1] if c + 1 < len(M.LL_BASE) else 1 << 17) and M.ll_bits(c) == M.LL_BITS[c]
    for ml in range(3, 8193):
        c = M.ml_code(ml - 3)
        assert M.ML_BASE[c] <= ml < M.ML_BASE[c + 1] and M.ml_bits(c) == M.ML_BITS[c]
    # the predefined tables are the decoder's: every state of an encoding table is the decoding cell of its symbol
    for t, norm, log in ((M.LL_T, M.LL_NORM, 6), (M.ML_T, M.ML_NORM, 6), (M.OF_T, M.OF_NORM, 5)):
        dec = R.fse_table(norm, log)
        for sym in range(len(norm)):
            cells = [u for u, (s, _nb, _base) in enumerate(dec) if s == sym]
            first = t.delta_state[sym] + (1 if abs(norm[sym]) == 1 else abs(norm[sym]))
            assert sorted(st - (1 << log) for st in t.state[first:first + len(cells)]) == cells, sym


# ---- sizes: which kZsMinMatch ---------------------------------------------------------------------------------------------------------
# Measured (this test prints the table). Frames with matches of at least m bytes, per slice and rung, in bytes:
#   slice, rung     literal-only  libzstd 1   m=4     m=5     m=6     m=8     m=12
#   lidar 8000, 0      34641       34641     34766   34656   34648   34641   34641
#   lidar 8000, 1      40477       40470     40747   40486   40479   40477   40477
#   lidar 8000, 2      37056       36753     37284   36997   37056   37056   37056
#   lidar 8000, 3      28997       28997     29190   29033   29008   28998   28997
#   lidar 8000, 4      21898       21905     22895   22194   21991   21892   21895
#   dds 6000, 0        29408       15374     16125   16175   16272   16397   16467
#   dds 6000, 1        34785       18251     18950   19151   19326   19431   19516
#   dds 6000, 2        32033       16900     17481   17604   17760   17857   17950
#   dds 6000, 3        25176       12796     14227   13902   13950   14064   14134
#   dds 6000, 4        21066        9986     12329   11745   11688   11817   11898
# The rule: the smallest DDS total among the values for which no lidar rung exceeds its literal-only frame. 4, 5 and 6 exceed on
# rung 0, 8 exceeds on rung 3 by one byte; 12 is the only one that qualifies (DDS total 79965 against 132468 literal-only and
# 73307 of libzstd level 1).
# Lidar ratios to the literal-only frames with m = 12: 0.99986 .. 1.00000; the assertion is that range widened by 0.02.
# DDS ratios to libzstd level 1 with m = 12: 1.0621 .. 1.1915 (literal-only: 1.895 .. 2.110); recorded, not bounded.
LIDAR_RATIOS = (0.99986, 1.00000)


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
            lit = theirs = 0
            ours = {m: 0 for m in M.CANDIDATES}
            o = 0
            while o < stream.size:
                n = int.from_bytes(stream[o:o + 4].tobytes(), "little")
                payload = stream[o + 4:o + 4 + n]
                o += 4 + n
                lz = oracle.lz4_trace(payload, M.SUB, M.HASH_BITS, M.MAX_MATCHES)
                lit += len(L.frame(payload))
                theirs += zstd_level1_size(payload.tobytes())
                for m in M.CANDIDATES:
                    frame = M.frame_info(payload, None, m, lz)
                    assert zstd_decompress(frame, n) == payload.tobytes()
                    ours[m] += len(frame)
            rows.append((name, c, lit, theirs, ours))
    return rows


def choose_min_match(rows):
    lidar = [r for r in rows if r[0] == SLICES[0]]
    dds = [r for r in rows if r[0] == SLICES[1]]
    ok = [m for m in M.CANDIDATES if all(r[4][m] <= r[2] for r in lidar)]
    if ok:
        return min(ok, key=lambda m: sum(r[4][m] for r in dds))
    return min(M.CANDIDATES, key=lambda m: max(r[4][m] / r[2] for r in lidar))


def test_frame_sizes_and_the_choice_of_the_shortest_kept_match(oracle):
    rows = size_rows(oracle)
    print("slice rung literal-only libzstd-1 " + " ".join(f"m={m}" for m in M.CANDIDATES))
    for name, c, lit, theirs, ours in rows:
        print(f"{name} {c} {lit} {theirs} " + " ".join(str(ours[m]) for m in M.CANDIDATES) +
              f"   m={M.MIN_MATCH}: / literal-only {ours[M.MIN_MATCH] / lit:.5f}, / libzstd {ours[M.MIN_MATCH] / theirs:.4f}")
    assert len(rows) == 10 and M.MIN_MATCH in M.CANDIDATES
    assert choose_min_match(rows) == M.MIN_MATCH
    for name, c, lit, theirs, ours in rows:
        mine = ours[M.MIN_MATCH]
        if name == SLICES[1]:
            assert mine < lit, (name, c, mine, lit)                                # every DDS rung gains
        else:
            assert LIDAR_RATIOS[0] - 0.02 <= mine / lit <= LIDAR_RATIOS[1] + 0.02, (name, c, mine / lit)


# ---- the shared header, under sanitizers ----------------------------------------------------------------------------------------------
def test_shared_header_matches_the_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "zstd_seq_code_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "zstd_seq_code_cli.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())
    assert int(next(lines)) == M.MIN_MATCH
    tabs = [M.OF_T, M.ML_T, M.LL_T]                                                # kZsTabOf, kZsTabMl, kZsTabLl
    norms = [M.OF_NORM, M.ML_NORM, M.LL_NORM]
    for w, (t, norm) in enumerate(zip(tabs, norms)):
        assert next(lines).split() == ["T", str(w), str(t.log)]
        for s in range(len(norm)):
            assert list(map(int, next(lines).split())) == [t.delta_nb[s], t.delta_state[s]], (w, s)
        assert list(map(int, next(lines).split())) == t.state, w
    for ll in range(131072):
        assert next(lines) == f"L {ll} {M.ll_code(ll)} {M.ll_bits(M.ll_code(ll))}"
    for ml in range(3, 8193):
        assert next(lines) == f"M {ml} {M.ml_code(ml - 3)} {M.ml_bits(M.ml_code(ml - 3))}"
    for off in range(1, 8192):
        assert next(lines) == f"O {off} {off + 3} {M.highbit(off + 3)}"
    n_x = n_s = 0
    for line in lines:
        p = line.split()
        if p[0] == "X":
            ll, ml, off, v, n = map(int, p[1:])
            want_v = want_n = 0
            for val, nb in M.sequence_fields(ll, ml, off)[3]:
                want_v |= val << want_n
                want_n += nb
            assert (v, n) == (want_v, want_n), line
            n_x += 1
        elif p[0] == "I":
            w, s, st = map(int, p[1:])
            assert st == tabs[w].init_state(s), line
        else:
            assert p[0] == "S"
            w, st, s, bits, nb, nxt = map(int, p[1:])
            assert (bits, nb, nxt) == tabs[w].step(st, s), line
            n_s += 1
    assert n_x > 500 and n_s == 64 * 36 + 64 * 53 + 32 * 29
