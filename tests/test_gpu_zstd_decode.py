"""ZSTD frames without sequences decoded on the device (cloudini_amd/csrc/zstd_decode.hip) through cldn_hip_zstd_decompress.

Expected values never come from the code under test: payloads are what went into the writers, verdicts and bytes are those of
tests/zstd_lit_rules.py (pinned one-sidedly against the system libzstd on the CPU, tests/test_zstd_lit_rules.py), the
inputs are tests/zstd_decode_cases.py's. Every output span lies between two guard spans of 64 bytes 0xA5."""
import os

import numpy as np
import pytest

import zstd_decode_cases as K
import zstd_lit_model as M
import zstd_lit_rules as R
from cloudini_amd import synth

GUARD = 64
FILL = 0xA5
CORRUPT, HOST = 0xFFFFFFFF, 0xFFFFFFFE
ERR_UNSUPPORTED, ERR_CORRUPT = -3, -6
EMPTY = M.frame(b"")                                     # a guard is the span of an empty frame: it decodes to nothing


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_libraries_export_the_calls_and_the_switch_defaults_to_off():
    from cloudini_amd import api, native
    for name in ("cldn_hip_zstd_decompress", "cldn_hip_decode_zstd"):
        assert hasattr(native.lib(), name), name
    for name in ("cldn_amd_device_zstd_decode", "cldn_amd_set_device_zstd_decode", "cldn_amd_device_zstd_decode_count"):
        assert hasattr(api.lib(), name), name
    assert api.device_zstd_decode() is False
    try:
        assert api.set_device_zstd_decode(True) is True and api.device_zstd_decode() is True
    finally:
        assert api.set_device_zstd_decode(False) is False
    assert api.device_zstd_decode() is False
    for name in ("zstd_decompress_host", "zstd_decompress_device", "decode_zstd_host", "decode_zstd_device"):
        assert hasattr(native.Codec, name), name


def test_decode_route_with_zstd_lists_the_new_kernels(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "zstd_route_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "cloudini_amd", "csrc"), "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "zstd_route_cli.cpp"), "-o", exe], check=True)
    rows = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    plain, lz4, zstd, empty = (r.split() for r in rows)
    assert "k_zstd_walk" not in plain and "k_lz4_decode_chunks" not in plain
    assert lz4 == plain[:1] + ["k_lz4_decode_chunks"] + plain[1:]                   # (routes of existing calls do not change)
    assert zstd == plain[:1] + ["k_zstd_walk", "k_zstd_decode_blocks"] + plain[1:]
    assert "k_zstd_walk" not in empty


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _codec():
    from cloudini_amd import native
    info, _ = synth.lidar_xyzi(10)
    return native.Codec(native.Plan(info))


def _run_device(codec, cases, r_in=0, r_out=0):
    """cases: [(frame, capacity)] through cldn_hip_zstd_decompress on DEVICE buffers, guards in front of and behind every
    output span. Input and output start r_in / r_out bytes behind a 256-byte boundary. Returns (sizes, [span bytes], error
    code of status() or 0) after checking every guard."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    frames, caps = [], []
    for frame, cap in cases:
        frames += [EMPTY, bytes(frame)]
        caps += [GUARD, int(cap)]
    frames.append(EMPTY)
    caps.append(GUARD)
    bo = np.zeros(len(frames) + 1, dtype=np.uint64)
    bo[1:] = np.cumsum([len(b) for b in frames])
    oo = np.zeros(len(frames) + 1, dtype=np.uint64)
    oo[1:] = np.cumsum(caps)
    data = np.frombuffer(b"".join(frames), dtype=np.uint8)
    d_in = torch.zeros(256 + data.size + 256, dtype=torch.uint8, device=dev)
    base_in = (-d_in.data_ptr()) % 256 + r_in
    d_in[base_in:base_in + data.size] = torch.from_numpy(data.copy()).to(dev)
    total = int(oo[-1])
    d_out = torch.full((512 + total + 512,), FILL, dtype=torch.uint8, device=dev)
    base_out = (-d_out.data_ptr()) % 256 + 256 + r_out
    d_sizes = torch.full((len(frames),), 0x77777777, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.zstd_decompress_device(d_in.data_ptr() + base_in, bo, d_out.data_ptr() + base_out, oo, d_sizes.data_ptr())
    code = 0
    try:
        codec.status()
    except native.CloudiniHipError as e:
        code = e.code
    out = d_out.cpu().numpy()
    sizes = d_sizes.cpu().numpy().view(np.uint32)
    assert np.all(out[:base_out] == FILL) and np.all(out[base_out + total:] == FILL)   # nothing outside the batch's spans
    spans = []
    for k in range(len(frames)):
        span = out[base_out + int(oo[k]):base_out + int(oo[k + 1])]
        if k % 2 == 0:
            assert sizes[k] == 0 and np.all(span == FILL), f"guard {k // 2} touched"
        else:
            spans.append(span)
    return sizes[1::2], spans, code


def _check_against_rules(cases, sizes, spans, code, labels):
    worst = R.OK
    for k, (frame, cap) in enumerate(cases):
        verdict, want = R.decode(frame, cap)
        worst = R.worst(worst, verdict)
        if verdict == R.OK:
            assert sizes[k] == len(want), labels[k]
            assert spans[k][:len(want)].tobytes() == want, labels[k]
            assert np.all(spans[k][len(want):] == FILL), labels[k]           # bytes behind the decoded ones keep their content
        else:
            assert sizes[k] == (HOST if verdict == R.HOST else CORRUPT), (labels[k], verdict, hex(int(sizes[k])))
            if R.walk(frame, cap)[0] != R.OK:                                # a verdict of the headers: the span is untouched
                assert np.all(spans[k] == FILL), labels[k]
    assert code == {R.OK: 0, R.HOST: ERR_UNSUPPORTED, R.CORRUPT: ERR_CORRUPT}[worst]


def _grid_cases(reverse=False):
    g = K.grid_frames()
    g = g[::-1] if reverse else g
    return [(f, c) for _n, f, c, _p in g], [n for n, *_ in g], [p for *_x, p in g]


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("r_in,r_out", [(0, 0), (1, 7), (15, 15)])
def test_zstd_decompress_block_grid(r_in, r_out, reverse):
    cases, labels, payloads = _grid_cases(reverse)
    codec = _codec()
    sizes, spans, code = _run_device(codec, cases, r_in, r_out)
    codec.close()
    assert code == 0
    for k, p in enumerate(payloads):                                         # the payloads that went into the writer
        assert sizes[k] == len(p) and spans[k].tobytes() == p, labels[k]
    _check_against_rules(cases, sizes, spans, code, labels)


@pytest.mark.gpu
def test_zstd_decompress_block_grid_at_every_output_residue():
    cases, labels, payloads = _grid_cases()
    cases, labels, payloads = cases[3::10], labels[3::10], payloads[3::10]
    # (with the frames the writer's own alignment cases name, whatever the stride picks)
    for n, f, c, p in K.grid_frames():
        if n.split("/")[0] in ("skewed_16383", "three_byte_last_block") and n not in labels:
            cases.append((f, c)), labels.append(n), payloads.append(p)
    codec = _codec()
    for r in range(16):
        sizes, spans, code = _run_device(codec, cases, (r * 7) % 16, r)
        assert code == 0
        for k, p in enumerate(payloads):
            assert sizes[k] == len(p) and spans[k].tobytes() == p, (r, labels[k])
    codec.close()


@pytest.mark.gpu
def test_zstd_decompress_block_grid_from_host_buffers():
    g = K.grid_frames()
    codec = _codec()
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


@pytest.mark.gpu
def test_zstd_decompress_foreign_and_mixed_frames():
    """libzstd's own frames and the hand-built ones in one batch: literal-only frames decode (treeless blocks included), frames
    with sequences or options get 0xfffffffe, leave their spans untouched and do not disturb their neighbours."""
    rows = [(n, f, c) for n, f, c, _p in K.libzstd_frames() + K.hand_frames()]
    verdicts = [R.decode(f, c)[0] for _n, f, c in rows]
    assert any(v == R.OK and n.startswith("treeless/") for (n, _f, _c), v in zip(rows, verdicts))
    assert any(v == R.OK and n == "geometric/level1/300000" for (n, _f, _c), v in zip(rows, verdicts))
    codec = _codec()
    # OK and HOST frames only: the call reports UNSUPPORTED
    some = [(r, v) for r, v in zip(rows, verdicts) if v != R.CORRUPT]
    assert sum(1 for _r, v in some if v == R.HOST) >= 10
    cases = [(f, c) for (_n, f, c), _v in some]
    sizes, spans, code = _run_device(codec, cases, 3, 9)
    assert code == ERR_UNSUPPORTED
    _check_against_rules(cases, sizes, spans, code, [n for (n, _f, _c), _v in some])
    # everything: a refused frame outranks it
    cases = [(f, c) for _n, f, c in rows]
    sizes, spans, code = _run_device(codec, cases, 0, 1)
    assert code == ERR_CORRUPT
    _check_against_rules(cases, sizes, spans, code, [n for n, _f, _c in rows])
    codec.close()


@pytest.mark.gpu
def test_zstd_decompress_capacity_takes_part_in_the_verdict():
    g = [x for x in K.grid_frames() if x[2]][::4]
    cases = [(f, c - 1) for _n, f, c, _p in g] + [(f, c) for _n, f, c, _p in g]
    labels = [n + "-1" for n, *_ in g] + [n for n, *_ in g]
    codec = _codec()
    sizes, spans, code = _run_device(codec, cases, 0, 5)
    codec.close()
    assert all(s == CORRUPT for s in sizes[:len(g)]) and [int(s) for s in sizes[len(g):]] == [c for _n, _f, c, _p in g]
    _check_against_rules(cases, sizes, spans, code, labels)


@pytest.mark.gpu
@pytest.mark.parametrize("base", range(10))
def test_zstd_decompress_damaged_frames(base):
    """tests/zstd_decode_cases.py's damage of one base frame -- every single-byte change (all 255 other values) of the header
    bytes the walk reads (frame header, block and literals headers, tree description, jump table, sequences byte), every
    truncation, random byte damage from a fresh seed -- against the rules' verdict and bytes; a refused frame's neighbours
    decode (an intact frame follows every 25th case)."""
    assert len(K.damage_bases()) == 10
    seed = int.from_bytes(os.urandom(4), "little") | 1
    cases = K.damaged_base(base, seed)
    intact = K.grid_frames()[5]
    codec = _codec()
    per_call = 4000
    for at in range(0, len(cases), per_call):
        part = cases[at:at + per_call]
        batch, labels = [], []
        for k, (n, f, c) in enumerate(part):
            batch.append((f, c)), labels.append(f"seed {seed} {n}")
            if k % 25 == 24:
                batch.append((intact[1], intact[2])), labels.append("intact")
        sizes, spans, code = _run_device(codec, batch, at % 16, (at // per_call * 5) % 16)
        _check_against_rules(batch, sizes, spans, code, labels)
    codec.close()


@pytest.mark.gpu
def test_zstd_decompress_more_blocks_than_the_workspace_is_host():
    """1500 Raw blocks of one byte in 6 KB of frame: a frame gets 2 block records, one per 256 source bytes and one per 128 KiB
    of capacity (R.record_limit), so this frame needs the host; its neighbours decode."""
    body = b"".join(M.block_header(k == 1499, 0, 1) + bytes([k & 255]) for k in range(1500))
    many = K.frame_header(1500) + body
    assert R.walk(many, 1500)[0] == R.OK and len(R.walk(many, 1500)[1]) == 1500 and R.decode(many, 1500)[0] == R.HOST
    assert K.libzstd_decompress(many, 1500) == bytes(k & 255 for k in range(1500))
    n, f, c, p = K.grid_frames()[7]
    cases = [(f, c), (many, 1500), (f, c)]
    codec = _codec()
    sizes, spans, code = _run_device(codec, cases, 0, 0)
    codec.close()
    assert code == ERR_UNSUPPORTED and [int(s) for s in sizes] == [c, HOST, c]
    assert spans[0].tobytes() == p and spans[2].tobytes() == p and np.all(spans[1] == FILL)


# ---- the arguments either decompress call refuses: the code and the text of cldn_hip_last_error, in the order of the checks ------
ERR_ARG = -1
_SPAN_2GIB = 1 << 31


def _refused_arguments():
    """(label, overrides of a valid one-span HOST call, return code, error text with {who} for lz4 / zstd)"""
    return [
        ("source tag", dict(src_loc=7), ERR_ARG, "invalid memory location tag"),
        ("output tag", dict(out_loc=7), ERR_ARG, "invalid memory location tag"),
        ("no source offsets", dict(src_offsets=None), ERR_ARG, "{who}_decompress: NULL offsets / sizes"),
        ("no output offsets", dict(out_offsets=None), ERR_ARG, "{who}_decompress: NULL offsets / sizes"),
        ("no sizes", dict(sizes=None), ERR_ARG, "{who}_decompress: NULL offsets / sizes"),
        ("device sizes at an odd address", dict(out_loc=1, sizes_shift=1), ERR_ARG, "{who}_decompress: device sizes must be 4-byte aligned"),
        ("descending source offsets", dict(src_offsets=[5, 1]), ERR_ARG, "{who}_decompress: offsets must be ascending"),
        ("descending output offsets", dict(out_offsets=[9, 4]), ERR_ARG, "{who}_decompress: offsets must be ascending"),
        ("source span of 2 GiB", dict(src=None, out=None, src_offsets=[0, _SPAN_2GIB], out_offsets=[0, 0]), ERR_UNSUPPORTED,
         "{who}_decompress: block or output span of more than 2 GiB"),
        ("output span of 2 GiB", dict(src=None, out=None, src_offsets=[0, 0], out_offsets=[7, 7 + _SPAN_2GIB]), ERR_UNSUPPORTED,
         "{who}_decompress: block or output span of more than 2 GiB"),
        ("no source", dict(src=None), ERR_ARG, "{who}_decompress: NULL buffer"),
        ("no output", dict(out=None), ERR_ARG, "{who}_decompress: NULL buffer"),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("who", ["lz4", "zstd"])
def test_decompress_calls_refuse_arguments_with_their_code_and_text(who):
    """None of these reaches a kernel: every check lies in front of the call's first device work."""
    import ctypes as C
    from cloudini_amd import native
    codec = _codec()
    fn = getattr(native.lib(), f"cldn_hip_{who}_decompress")
    u64p = C.POINTER(C.c_uint64)

    def call(src_loc=0, out_loc=0, src=b"\0", out=b"\0\0\0\0", src_offsets=(0, 1), out_offsets=(0, 4), sizes=True, sizes_shift=0, n=1):
        src_a = None if src is None else np.frombuffer(src, dtype=np.uint8).copy()
        out_a = None if out is None else np.frombuffer(out, dtype=np.uint8).copy()
        so = None if src_offsets is None else np.array(src_offsets, dtype=np.uint64)
        oo = None if out_offsets is None else np.array(out_offsets, dtype=np.uint64)
        sz = np.zeros(2, dtype=np.uint32) if sizes else None
        rc = fn(codec._h, None if src_a is None else src_a.ctypes.data, src_loc, None if so is None else so.ctypes.data_as(u64p), n,
                None if out_a is None else out_a.ctypes.data, out_loc, None if oo is None else oo.ctypes.data_as(u64p),
                None if sz is None else sz.ctypes.data + sizes_shift)
        return rc, native.lib().cldn_hip_last_error().decode()

    for label, overrides, code, text in _refused_arguments():
        assert call(**overrides) == (code, text.format(who=who)), label
    # no spans: OK whatever else is missing
    assert call(n=0, src=None, out=None, src_offsets=None, out_offsets=None, sizes=None)[0] == 0
    codec.close()
