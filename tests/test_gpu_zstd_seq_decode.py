"""ZSTD frames WITH sequences decoded on the device (cloudini_amd/csrc/zstd_seq_decode.hip) through cldn_hip_zstd_decompress,
behind cldn_hip_codec_set_zstd_sequences.

Expected values never come from the code under test: payloads are what went into the compressors (or, for the constructed
grid, what tests/zstd_seq_cases.py's expand() makes of the sequences), verdicts and bytes are those of tests/zstd_seq_rules.py
(pinned one-sidedly against the system libzstd on the CPU, tests/test_zstd_seq_rules.py). Every output span lies between two
guard spans of 64 bytes 0xA5 (test_gpu_zstd_decode._run_device)."""
import os
import subprocess

import numpy as np
import pytest

import zstd_decode_cases as K
import zstd_seq_cases as Q
import zstd_seq_rules as S
from test_gpu_zstd_decode import CORRUPT, ERR_CORRUPT, ERR_UNSUPPORTED, FILL, GUARD, HOST, _codec, _run_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_library_exports_the_switch_and_it_defaults_to_off():
    from cloudini_amd import native
    for name in ("cldn_hip_codec_set_zstd_sequences", "cldn_hip_codec_zstd_sequences"):
        assert hasattr(native.lib(), name), name
    assert hasattr(native.Codec, "set_zstd_sequences") and hasattr(native.Codec, "zstd_sequences")
    assert native.lib().cldn_hip_codec_zstd_sequences(None) == 0


def test_decode_route_with_zstd_seq_lists_the_new_kernels(tmp_path):
    exe = str(tmp_path / "zstd_seq_route_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "cloudini_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "zstd_seq_route_cli.cpp"), "-o", exe], check=True)
    rows = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    zstd, seq, empty = (r.split() for r in rows)
    assert "k_zstd_seq_decode" not in zstd and "k_zstd_seq_exec" not in zstd
    at = zstd.index("k_zstd_decode_blocks") + 1
    assert seq == zstd[:at] + ["k_zstd_seq_decode", "k_zstd_seq_exec"] + zstd[at:]
    assert "k_zstd_seq_decode" not in empty and "k_zstd_walk" not in empty


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _seq_codec(on=True):
    codec = _codec()
    assert codec.zstd_sequences() is False
    codec.set_zstd_sequences(on)
    assert codec.zstd_sequences() is on
    return codec


_verdicts = {}


def _decode(frame, cap):
    """S.decode, computed once per frame and capacity"""
    if (frame, cap) not in _verdicts:
        _verdicts[(frame, cap)] = S.decode(frame, cap)
    return _verdicts[(frame, cap)]


def _check_against_rules(cases, sizes, spans, code, labels):
    worst = S.OK
    for k, (frame, cap) in enumerate(cases):
        verdict, want = _decode(frame, cap)
        worst = S.worst(worst, verdict)
        if verdict == S.OK:
            assert sizes[k] == len(want), labels[k]
            assert spans[k][:len(want)].tobytes() == want, labels[k]
            assert np.all(spans[k][len(want):] == FILL), labels[k]           # bytes behind the decoded ones keep their content
        else:
            assert sizes[k] == (HOST if verdict == S.HOST else CORRUPT), (labels[k], verdict, hex(int(sizes[k])))
    assert code == {S.OK: 0, S.HOST: ERR_UNSUPPORTED, S.CORRUPT: ERR_CORRUPT}[worst]


@pytest.mark.gpu
def test_frames_with_sequences_need_the_switch():
    """off (the default): 0xfffffffe and an untouched span, as before the switch existed; on: the bytes"""
    rows = [x for x in Q.libzstd_frames() if x[0] in ("zipf/level1/40000", "zipf/level3/5000", "text/level1")]
    assert len(rows) == 3 and all(S.decode_trace(f, c)[2]["has_seq"] for _n, f, c, _p in rows)
    cases = [(f, c) for _n, f, c, _p in rows]
    codec = _codec()
    sizes, spans, code = _run_device(codec, cases, 0, 3)
    assert code == ERR_UNSUPPORTED and all(s == HOST for s in sizes) and all(np.all(sp == FILL) for sp in spans)
    codec.set_zstd_sequences(True)
    sizes, spans, code = _run_device(codec, cases, 0, 3)
    assert code == 0
    for k, (n, _f, c, p) in enumerate(rows):
        assert sizes[k] == c and spans[k].tobytes() == p, n
    codec.set_zstd_sequences(False)
    sizes, spans, code = _run_device(codec, cases, 0, 3)
    codec.close()
    assert code == ERR_UNSUPPORTED and all(s == HOST for s in sizes) and all(np.all(sp == FILL) for sp in spans)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("r_in,r_out", [(0, 0), (1, 7), (15, 15)])
def test_constructed_grid(r_in, r_out, reverse):
    g = Q.grid_frames()[::-1] if reverse else Q.grid_frames()
    cases, labels = [(f, c) for _n, f, c, _p in g], [n for n, *_ in g]
    codec = _seq_codec()
    sizes, spans, code = _run_device(codec, cases, r_in, r_out)
    codec.close()
    for k, (n, _f, c, p) in enumerate(g):                                    # what expand() made of the sequences
        if p is not None:
            assert sizes[k] == len(p) and spans[k][:len(p)].tobytes() == p, n
    _check_against_rules(cases, sizes, spans, code, labels)


@pytest.mark.gpu
def test_alignment_cases_at_every_output_residue_and_from_host_buffers():
    g = [x for x in Q.grid_frames() if x[0].startswith(("align/", "match/", "rep/", "ring/"))]
    cases = [(f, c) for _n, f, c, _p in g]
    codec = _seq_codec()
    for r in range(16):
        sizes, spans, code = _run_device(codec, cases, (r * 7) % 16, r)
        assert code == 0
        for k, (n, _f, _c, p) in enumerate(g):
            assert sizes[k] == len(p) and spans[k].tobytes() == p, (r, n)
    caps = [c + GUARD for _n, _f, c, _p in g]
    out = np.full(sum(caps), FILL, np.uint8)
    out, sizes, rc = codec.zstd_decompress_host([f for _n, f, _c, _p in g], caps, out)
    codec.close()
    assert rc == 0
    at = 0
    for (n, _f, c, p), cap in zip(g, caps):
        assert out[at:at + c].tobytes() == p and np.all(out[at + c:at + cap] == FILL), n
        at += cap
    assert [int(s) for s in sizes] == [c for _n, _f, c, _p in g]


def _mixed_batch(rows, judge_rows=True):
    """every frame of rows followed by a neighbour: in turn a frame the device hands to the host and a literal-only one"""
    old = [(n, f, c, None, _decode(f, c)[0]) for n, f, c, _p in K.hand_frames() + K.libzstd_frames() if c <= 40000]
    host = [x[:4] for x in old if x[4] == S.HOST]
    lit = [x[:4] for x in old if x[4] == S.OK and not S.decode_trace(x[1], x[2])[2]["has_seq"]]
    assert len(host) >= 5 and len(lit) >= 5
    mixed = []
    for k, row in enumerate(rows):
        mixed.append(row)
        mixed.append((host if k % 2 == 0 else lit)[(k // 2) % len(host if k % 2 == 0 else lit)])
    return mixed, [_decode(f, c)[0] for _n, f, c, _p in mixed] if judge_rows else None


@pytest.mark.gpu
def test_libzstd_frames_next_to_literal_only_and_host_frames(oracle):
    """ALL of set (b), each frame followed by a neighbour. What a frame of (b) must give is known without the model: the bytes
    that went into the compressor (tests/test_zstd_seq_rules.py holds the model to the same on the CPU), or for the named
    exceptions of Q.LIBZSTD_HOST 0xfffffffe and an untouched span. The neighbours (small) are held to the model."""
    rows = Q.libzstd_frames() + Q.lidar_frames(oracle)
    mixed, _v = _mixed_batch(rows, judge_rows=False)
    cases = [(f, c) for _n, f, c, _p in mixed]
    codec = _seq_codec()
    sizes, spans, code = _run_device(codec, cases, 3, 9)
    codec.close()
    assert code == ERR_UNSUPPORTED
    for k, (n, f, c, p) in enumerate(mixed):
        if k % 2 == 0 and n in Q.LIBZSTD_HOST:
            assert sizes[k] == HOST and np.all(spans[k] == FILL), n
        elif k % 2 == 0:
            assert sizes[k] == c and spans[k].tobytes() == p, n
        else:
            verdict, want = _decode(f, c)
            if verdict == S.OK:
                assert sizes[k] == len(want) and spans[k][:len(want)].tobytes() == want and np.all(spans[k][len(want):] == FILL), n
            else:
                assert verdict == S.HOST and sizes[k] == HOST and np.all(spans[k] == FILL), n     # (verdicts of the headers)


@pytest.mark.gpu
def test_capacity_takes_part_in_the_verdict():
    g = [x for x in Q.grid_frames() if x[3]][::5] + [x for x in Q.libzstd_frames() if x[0] in ("zipf/level3/5000", "zipf/level1/5000")]
    cases = [(f, c - 1) for _n, f, c, _p in g] + [(f, c) for _n, f, c, _p in g]
    labels = [n + "-1" for n, *_ in g] + [n for n, *_ in g]
    codec = _seq_codec()
    sizes, spans, code = _run_device(codec, cases, 0, 5)
    codec.close()
    assert all(s == CORRUPT for s in sizes[:len(g)]) and [int(s) for s in sizes[len(g):]] == [c for _n, _f, c, _p in g]
    _check_against_rules(cases, sizes, spans, code, labels)


@pytest.mark.gpu
@pytest.mark.parametrize("base", range(8))
def test_damaged_frames(base):
    """tests/zstd_seq_cases.py's damage of one base frame -- every single-byte change of the bytes the new walk reads (count,
    modes byte, table descriptions, RLE bytes), flips in the last 8 bytes of the bit stream, every truncation, and this base's
    share of the 300 random changes -- against the rules' verdict and bytes; an intact frame follows every 25th case."""
    assert len(Q.damage_bases()) == 8
    cases = Q.damaged_base(base) + [c for c in Q.random_damage() if c[0].startswith(f"{base}/")]
    intact = Q.grid_frames()[5]
    codec = _seq_codec()
    per_call = 4000
    for at in range(0, len(cases), per_call):
        batch, labels = [], []
        for k, (n, f, c) in enumerate(cases[at:at + per_call]):
            batch.append((f, c)), labels.append(n)
            if k % 25 == 24:
                batch.append((intact[1], intact[2])), labels.append("intact")
        sizes, spans, code = _run_device(codec, batch, at % 16, (at // per_call * 5) % 16)
        _check_against_rules(batch, sizes, spans, code, labels)
    codec.close()
