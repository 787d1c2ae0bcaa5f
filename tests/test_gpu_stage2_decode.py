"""The decode direction of the batch transcoder with stage 2 undone on the device (TranscodeOptions::device_stage2_decode,
`cloudini_batch_transcode --decode --device-stage2`, api.decode_directory(device_stage2=True)) and the two calls behind it,
cldn_hip_decode_lz4_gather / cldn_hip_decode_zstd_gather.

The contract: every output file is the file of a run without the option, byte for byte, and every error is the same error.
Expected bytes never come from the code under test: the messages are built on the CPU (tests/stage2_decode_cases.py: the
oracle's stage-1 streams, libzstd level 1 / liblz4), the points they decode to are the clouds' own where the schema is
lossless, the option-off run is the path the reference's converter pins (tests/test_batch_transcoder.py), and where the
compiled reference is present its decode is compared too. The "no fall-back" counters rest on the CPU precondition of
tests/test_stage2_decode_plan.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import lz4_block_rules as LR
import lz4_body
import stage2_decode_cases as S
import zstd_decode_cases as ZC
from cloudini_amd import api
from cloudini_amd.schema import CompressionOption

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
ERR_ARG, ERR_UNSUPPORTED, ERR_CORRUPT = -1, -3, -6
NEEDS_HOST, REFUSED = 0xFFFFFFFE, 0xFFFFFFFF
COUNTERS = ("device_stage2_chunks", "host_stage2_chunks", "device_stage2_retries")


def _write(folder, messages):
    os.makedirs(folder, exist_ok=True)
    for k, m in enumerate(messages):
        np.asarray(m, dtype=np.uint8).tofile(os.path.join(folder, f"msg_{k:05d}.bin"))


def _files(folder):
    if not os.path.isdir(folder):
        return {}
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def _reference():
    from oracle.binding import RefLib, ref_available
    return RefLib() if ref_available() else None


def _both(tmp_path, messages, batch=8, tag=""):
    """the directory through the transcoder without and with the option: (files, stats without, stats with); the files are equal"""
    src, off, on = str(tmp_path / f"in{tag}"), str(tmp_path / f"off{tag}"), str(tmp_path / f"on{tag}")
    _write(src, messages)
    st_off = api.decode_directory(src, off, batch_messages=batch)
    st_on = api.decode_directory(src, on, batch_messages=batch, device_stage2=True)
    want, got = _files(off), _files(on)
    assert sorted(want) == sorted(got) and len(want) == len(messages)
    for name in want:
        assert got[name] == want[name], name
    assert [int(st_off[k]) for k in COUNTERS] == [0, 0, 0]            # option off: the three counters are 0
    for k in ("messages", "points", "output_bytes", "gpu_batches"):
        assert st_on[k] == st_off[k], k
    return want, st_off, st_on


def _counters(st):
    return [int(st[k]) for k in COUNTERS]


@pytest.mark.parametrize("comp", S.COMPRESSIONS, ids=lambda c: c.name)
@pytest.mark.parametrize("family", S.FAMILIES)
def test_same_files_and_no_fall_back(tmp_path, oracle, family, comp):
    """8 messages of 0 .. 65537 points written the way the host encoder writes them: the same files, every chunk on the device"""
    msgs, sizes = S.directory(oracle, family, comp)
    # the host encoder writes these very streams (one message per directory is enough to tie the CPU precondition to them)
    info, data = S.cloud(family, 32769)
    info = info.copy(compression_opt=comp)
    stream = api.PointcloudEncoder(info).encode(data)
    body = msgs[4][2]
    assert sizes[4] == 32769 and stream[stream.size - body.size:].tobytes() == body.tobytes()
    files, _off, st = _both(tmp_path, [m for m, _p, _b in msgs])
    assert _counters(st) == [sum(S.chunks_of_points(n) for n in sizes), 0, 0] and _counters(st)[0] == 13
    ref = _reference()
    for k, (m, _p, _b) in enumerate(msgs):
        got = files[f"msg_{k:05d}.bin"]
        if ref is not None:
            assert got == ref.ros_decompress(m, len(got) + 4096).tobytes(), k
        if family == "raw16":   # raw copies: the points themselves lie in the output
            cloud = S.cloud(family, sizes[k])[1].tobytes()
            assert cloud == b"" or cloud in got


@pytest.mark.parametrize("writer", ["lz4", "lz4_fast", "zstd", "zstd_matches"])
def test_messages_of_the_device_writers(tmp_path, writer):
    """CLDN_HIP_STAGE2_LZ4, _LZ4_FAST, _ZSTD and _ZSTD with matches: their messages take the same way back, no fall-back"""
    comp = CompressionOption.LZ4 if writer.startswith("lz4") else CompressionOption.ZSTD
    sizes = [4096, 32769, 65537, 1, 32768, 65537]
    try:
        if comp == CompressionOption.LZ4:
            assert api.set_device_lz4(2 if writer == "lz4_fast" else 1) == (2 if writer == "lz4_fast" else 1)
        else:
            assert api.set_device_zstd(True) is True
            assert api.set_device_zstd_matches(writer == "zstd_matches") is (writer == "zstd_matches")
        msgs = []
        for k, n in enumerate(sizes):
            info, data = S.cloud("dds" if k % 2 else "xyzi_ring", n)
            info = info.copy(compression_opt=comp)
            msgs.append(S.compressed_message(info, api.PointcloudEncoder(info).encode(data), stamp=(1700000000, k)))
    finally:
        api.set_device_lz4(0)
        api.set_device_zstd_matches(False)
        api.set_device_zstd(False)
    _files_, _off, st = _both(tmp_path, msgs)
    assert _counters(st) == [sum(S.chunks_of_points(n) for n in sizes), 0, 0]


def test_a_batch_of_none_lz4_and_zstd_messages_of_two_schemas(tmp_path, oracle):
    plan = [("xyzi", 32769, CompressionOption.NONE), ("xyzi", 65537, CompressionOption.LZ4), ("xyzi", 4096, CompressionOption.LZ4),
            ("raw16", 32769, CompressionOption.ZSTD), ("xyzi", 1, CompressionOption.NONE), ("raw16", 65537, CompressionOption.ZSTD),
            ("raw16", 4096, CompressionOption.LZ4), ("xyzi", 32768, CompressionOption.ZSTD), ("xyzi", 0, CompressionOption.ZSTD)]
    msgs = [S.message_of(oracle, f, n, c, k)[0] for k, (f, n, c) in enumerate(plan)]
    for batch, tag in ((16, "a"), (4, "b")):
        _files_, _off, st = _both(tmp_path, msgs, batch=batch, tag=tag)
        want = sum(S.chunks_of_points(n) for _f, n, c in plan if c != CompressionOption.NONE)
        assert _counters(st) == [want, 0, 0] and want == 3 + 1 + 2 + 3 + 1 + 1


# ---- chunks the device hands back -------------------------------------------------------------------------------------------------
RAW4 = 4   # 4 UINT8 fields: a full chunk's payload is 131072 bytes, a size tests/zstd_decode_cases.py has frames for


def _raw4_message(chunk_frames, n_points, k=0):
    info = S.raw_info(n_points, RAW4).copy(compression_opt=CompressionOption.ZSTD)
    stream = np.concatenate([np.frombuffer(api.EncodeHeader(info), dtype=np.uint8), lz4_body.frame(chunk_frames)])
    return S.compressed_message(info, stream, stamp=(1700000000, k))


def _raw4_payloads():
    src = ZC.sources()
    a, b = src["geometric"][:131072], src["zipf"][:131072]
    return a, b, src["geometric"][200000:200000 + 4 * 100]


def _handed_back(kind):
    """a frame of the middle chunk's 131072 bytes that libzstd decodes and the device hands back"""
    payload = _raw4_payloads()[1]
    if kind == "checksum":
        frame = ZC.libzstd_compress(payload, ZC.LEVEL1 + ((ZC.C_CHECKSUM, 1),))
    else:  # a skippable frame in front of the frame (zstd_decode_cases.hand_frames' "host/skippable")
        frame = b"\x50\x2a\x4d\x18\x04\x00\x00\x00abcd" + ZC.libzstd_compress(payload, ZC.LEVEL1)
    assert ZC.libzstd_decompress(frame, 131072 + 64) == payload
    return frame


@pytest.mark.parametrize("place", [0, 1, 2], ids=["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["checksum", "skippable"])
def test_a_chunk_the_device_hands_back_goes_through_the_host_once(tmp_path, kind, place):
    a, b, tail = _raw4_payloads()
    level1 = lambda p: ZC.libzstd_compress(p, ZC.LEVEL1)
    special = _raw4_message([level1(a), _handed_back(kind), level1(tail)], 2 * 32768 + 100, k=9)
    plain = [_raw4_message([level1(a)], 32768, k=1), _raw4_message([level1(b), level1(tail)], 32768 + 100, k=2)]
    msgs = plain[:]
    msgs.insert(place, special)
    files, _off, st = _both(tmp_path, msgs)
    assert _counters(st) == [5, 1, 1]                                   # 6 chunks, one of them through the host, one retry
    assert (a + b + tail) in files[f"msg_{place:05d}.bin"]             # raw copies: the three chunks' bytes, in place


def _refused(kind):
    a, b, tail = _raw4_payloads()
    if kind == "zstd":
        comp = CompressionOption.ZSTD
        good = [ZC.libzstd_compress(p, ZC.LEVEL1) for p in (a, b, tail)]
        bad = good[1][:-7]                                             # a truncated frame
        assert ZC.libzstd_decompress(bad, 131072 + 64) is None
    else:
        comp = CompressionOption.LZ4
        good = [LR.lz4_compress(p) for p in (a, b, tail)]
        bad = good[1][:-9]                                             # the block ends inside its last literals
        assert LR.decode(bad, 131072 + 64) is None and LR.lz4_decompress_safe(bad, 131072 + 64) is None
    info = S.raw_info(2 * 32768 + 100, RAW4).copy(compression_opt=comp)
    head = np.frombuffer(api.EncodeHeader(info), dtype=np.uint8)
    msg = lambda frames, k: S.compressed_message(info, np.concatenate([head, lz4_body.frame(frames)]), stamp=(1700000000, k))
    return [msg(good, 0), msg([good[0], bad, good[2]], 1), msg(good, 2)]


@pytest.mark.parametrize("kind", ["zstd", "lz4"])
def test_a_chunk_both_sides_refuse_is_the_same_error(tmp_path, kind):
    msgs = _refused(kind)
    src = str(tmp_path / "in")
    _write(src, msgs)
    errors = []
    for on in (False, True):
        dst = str(tmp_path / ("on" if on else "off"))
        with pytest.raises(RuntimeError) as e:
            api.decode_directory(src, dst, batch_messages=8, device_stage2=on)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and ("decompression failed" in errors[0])
    assert set(_files(str(tmp_path / "on"))) <= set(_files(str(tmp_path / "off")))


# ---- the tool, a directory and a bag ----------------------------------------------------------------------------------------------
def test_the_tool_takes_the_option_for_a_directory_and_for_a_bag(tmp_path, oracle):
    import mcap_py
    msgs = [S.message_of(oracle, "xyzi_ring", n, CompressionOption.ZSTD, k)[0] for k, n in enumerate([32769, 4096, 65537])]
    src = str(tmp_path / "in")
    _write(src, msgs)
    outs = {}
    for flag in ([], ["--device-stage2"]):
        dst = str(tmp_path / ("d_on" if flag else "d_off"))
        r = subprocess.run([TOOL, src, dst, "--decode", "--batch", "4"] + flag, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        st = json.loads(r.stdout.strip().splitlines()[-1])
        assert [st[k] for k in COUNTERS] == ([6, 0, 0] if flag else [0, 0, 0])
        outs[bool(flag)] = _files(dst)
    assert outs[True] == outs[False] and len(outs[True]) == 3
    # a bag: the compressed clouds between other messages
    cpc2 = "point_cloud_interfaces/msg/CompressedPointCloud2"
    schemas = [(1, cpc2, "ros2msg", b"compressed_data"), (2, "std_msgs/msg/String", "ros2msg", b"string data")]
    channels = [(1, 1, "/lidar", "cdr", []), (2, 2, "/chatter", "cdr", [])]
    records, t = [], 100
    for k, m in enumerate(msgs):
        records.append((2, 2 * k, t, t, b"hello %d" % k)); t += 5
        records.append((1, 2 * k + 1, t, t, m.tobytes())); t += 5
    bag = str(tmp_path / "in.mcap")
    mcap_py.write(bag, "ros2", schemas, channels, records, chunk_messages=2)
    got = {}
    for flag in ([], ["--device-stage2"]):
        dst = str(tmp_path / ("on.mcap" if flag else "off.mcap"))
        r = subprocess.run([TOOL, bag, dst, "--decode", "--mcap-compression", "none", "--batch", "2"] + flag,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        st = json.loads(r.stdout.strip().splitlines()[-1])
        assert st["converted"] == 3 and [st[k] for k in COUNTERS] == ([6, 0, 0] if flag else [0, 0, 0])
        got[bool(flag)] = mcap_py.read(dst)["messages"]
    assert got[True] == got[False] and len(got[True]) == 6
    assert [d for ch, _s, _l, _p, d in got[True] if ch == 1] == [outs[False][f"msg_{k:05d}.bin"] for k in range(3)]


# ---- the two calls themselves -----------------------------------------------------------------------------------------------------
def _abi_batch(oracle, comp):
    """three clouds of 3, 0 and 2 chunks (xyzi_ring): info, clouds, bodies, payloads per chunk, chunk sizes"""
    from cloudini_amd import native
    sizes = [65537, 0, 32769]
    info = S.cloud("xyzi_ring", 65537)[0].copy(compression_opt=comp)
    clouds, bodies, payloads = [], [], []
    for n in sizes:
        _i, data = S.cloud("xyzi_ring", n)
        body, p = S.body_of(oracle, info, data, comp)
        clouds.append(data), bodies.append(body), payloads.extend(p)
    chunk_sizes = []
    for b in bodies:
        chunk_sizes += [c.size for c in lz4_body.chunks_of(b)]
    codec = native.Codec(native.Plan(info))
    codec.set_zstd_sequences(True)
    stage2 = native.STAGE2_LZ4 if comp == CompressionOption.LZ4 else native.STAGE2_ZSTD
    return codec, stage2, sizes, clouds, bodies, payloads, chunk_sizes


def _at_residue(body, residue):
    """the body's bytes at a host address with this residue modulo 16"""
    room = np.zeros(body.size + 64, dtype=np.uint8)
    shift = (residue - room.ctypes.data) % 16
    view = room[shift:shift + body.size]
    view[:] = body
    assert body.size == 0 or view.ctypes.data % 16 == residue
    return view


@pytest.mark.parametrize("comp", S.COMPRESSIONS, ids=lambda c: c.name)
def test_the_gather_calls(oracle, comp):
    from cloudini_amd import native
    codec, stage2, sizes, clouds, bodies, payloads, chunk_sizes = _abi_batch(oracle, comp)
    step = codec.plan.point_step
    want = [c.tobytes() for c in codec.decode_host([lz4_body.frame(payloads[:3]), np.zeros(0, np.uint8), lz4_body.frame(payloads[3:])], sizes)]
    assert [len(w) for w in want] == [n * step for n in sizes]
    contiguous = codec.decode_lz4_host(bodies, sizes) if comp == CompressionOption.LZ4 else codec.decode_zstd_host(bodies, sizes)
    assert [c.tobytes() for c in contiguous] == want
    sizes_of = [p.size for p in payloads]
    # expanded for none = the contiguous call on the gathered bytes; bodies at every address residue, with and without chunk_sizes
    for residue in (0, 1, 7, 15):
        placed = [_at_residue(b, residue) for b in bodies]
        for cs in (None, chunk_sizes):
            got, verdicts, rc = codec.decode_stage2_gather(stage2, placed, sizes, chunk_sizes=cs)
            assert rc == 0 and [g.tobytes() for g in got] == want, (residue, cs is None)
            assert verdicts.tolist() == sizes_of
    # expanded for every chunk = cldn_hip_decode_stage1 on the same payloads: the compressed bytes are not looked at
    junk = [lz4_body.frame([b"\xff" * c for c in chunk_sizes[:3]]), np.zeros(0, np.uint8), lz4_body.frame([b"\xff" * c for c in chunk_sizes[3:]])]
    got, verdicts, rc = codec.decode_stage2_gather(stage2, junk, sizes, chunk_sizes=chunk_sizes, expanded=payloads)
    assert rc == 0 and [g.tobytes() for g in got] == want and verdicts.tolist() == sizes_of
    # ... and for one chunk, whose compressed bytes are damaged
    damaged = [b.copy() for b in bodies]
    at = 4 + chunk_sizes[0] + 4                                                       # chunk 1: no LZ4 block (a literal run past
    damaged[0][at:at + chunk_sizes[1]] = 0xFF                                         # its end), no ZSTD frame (the magic)
    got, verdicts, rc = codec.decode_stage2_gather(stage2, damaged, sizes, chunk_sizes=chunk_sizes,
                                                   expanded=[None, payloads[1], None, None, None])
    assert rc == 0 and [g.tobytes() for g in got] == want and verdicts.tolist() == sizes_of
    # a payload above the slot capacity
    capacity = codec.plan.stage1_bound(32768) + 60
    too_long = [None] * 5
    too_long[3] = np.zeros(capacity + 1, dtype=np.uint8)
    _g, _v, rc = codec.decode_stage2_gather(stage2, bodies, sizes, chunk_sizes=chunk_sizes, expanded=too_long)
    assert rc == ERR_ARG
    too_long[3] = np.zeros(capacity, dtype=np.uint8)     # (a full slot is taken; zeros are no stage-1 stream of this chunk or are one:
    _g, _v, rc = codec.decode_stage2_gather(stage2, bodies, sizes, chunk_sizes=chunk_sizes, expanded=too_long)   # either way no ARG)
    assert rc in (0, ERR_CORRUPT)
    # a wrong chunk_sizes entry
    wrong = list(chunk_sizes)
    wrong[3] += 1
    _g, verdicts, rc = codec.decode_stage2_gather(stage2, bodies, sizes, chunk_sizes=wrong)
    assert rc == ERR_CORRUPT
    # verdicts are filled when the call fails: chunk 1 is damaged and not expanded
    out = np.full(sum(sizes) * step, 0xA5, dtype=np.uint8)
    _g, verdicts, rc = codec.decode_stage2_gather(stage2, damaged, sizes, chunk_sizes=chunk_sizes, out=out)
    assert rc in (ERR_CORRUPT, ERR_UNSUPPORTED) and (out == 0xA5).all()             # no point comes back from a failed call
    assert verdicts[1] in (NEEDS_HOST, REFUSED) and [int(v) for k, v in enumerate(verdicts) if k != 1] == [s for k, s in enumerate(sizes_of) if k != 1]
    assert codec.decode_stats() is not None
    codec.close()


def test_four_kinds_of_decode_call_share_the_staging_ring(oracle):
    """cldn_hip_lz4_decompress, a gather call (tables and expanded sizes: two slots), cldn_hip_zstd_decompress and
    cldn_hip_decode_lz4 stage their tables in the same ring of 4 page-locked buffers. One after the other on one codec, with
    no synchronisation added between them, the fifth upload waits for the first one's event: every call gives what it gives
    on a codec of its own, which is what the inputs were built from."""
    import torch
    from cloudini_amd import native, synth
    dev = torch.device("cuda", 0)
    LZ4, ZSTD = CompressionOption.LZ4, CompressionOption.ZSTD
    rs = np.random.RandomState(5)
    lits = [rs.randint(0, 256, 18).astype(np.uint8).tobytes() for _ in range(2)]
    blocks = [bytes([0xF0, 3]) + p for p in lits]                                   # one run of 18 literals: 20 bytes
    assert all(len(b) == 20 and LR.decode(b, 64) == p for b, p in zip(blocks, lits))
    texts = [bytes(rs.randint(0, 4, n).astype(np.uint8)) for n in (40, 100)]
    frames = [S.stage2(ZSTD, t) for t in texts]
    info = synth.lidar_xyzi(3)[0]
    clouds = [synth.lidar_xyzi(3, seed=300 + k)[1] for k in range(18)]
    bodies, payloads = {}, {}
    for comp, part in ((ZSTD, clouds[:9]), (LZ4, clouds[9:])):
        made = [S.body_of(oracle, info, c, comp) for c in part]
        bodies[comp], payloads[comp] = [b for b, _p in made], [p[0] for _b, p in made]
    want_points = {comp: [oracle.decode_stage1(info, lz4_body.frame([p]), 3, fill=0x5A) for p in payloads[comp]] for comp in (ZSTD, LZ4)}
    expanded = [None] * 9
    expanded[4] = payloads[ZSTD][4]

    def spans(parts, caps):
        data = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        so, oo = np.zeros(len(parts) + 1, dtype=np.uint64), np.zeros(len(parts) + 1, dtype=np.uint64)
        so[1:], oo[1:] = np.cumsum([len(p) for p in parts]), np.cumsum(caps)
        return (torch.from_numpy(data).to(dev), so, torch.full((int(oo[-1]),), 0xA5, dtype=torch.uint8, device=dev), oo,
                torch.full((len(parts),), 0x77777777, dtype=torch.int32, device=dev))

    def run(codecs):
        for c in codecs:
            c.set_zstd_sequences(True)
        b_in, b_so, b_out, b_oo, b_sizes = spans(blocks, [32, 32])
        f_in, f_so, f_out, f_oo, f_sizes = spans(frames, [64, 128])
        body = np.concatenate(bodies[LZ4])
        offs = np.zeros(10, dtype=np.uint64)
        offs[1:] = np.cumsum([b.size for b in bodies[LZ4]])
        d_body = torch.from_numpy(body).to(dev)
        d_points = torch.full((9 * 3 * info.point_step,), 0x5A, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        codecs[0].lz4_decompress_device(b_in.data_ptr(), b_so, b_out.data_ptr(), b_oo, b_sizes.data_ptr())
        got, verdicts, rc = codecs[1].decode_stage2_gather(native.STAGE2_ZSTD, bodies[ZSTD], [3] * 9, expanded=expanded,
                                                           out=np.full(9 * 3 * info.point_step, 0x5A, dtype=np.uint8))
        codecs[2].zstd_decompress_device(f_in.data_ptr(), f_so, f_out.data_ptr(), f_oo, f_sizes.data_ptr())
        codecs[3].decode_lz4_device(d_body.data_ptr(), offs, np.full(9, 3, dtype=np.uint64), d_points.data_ptr(), d_points.numel())
        for c in set(codecs):
            c.synchronize()
            c.status()
        return (b_out.cpu().numpy().tobytes(), b_sizes.cpu().tolist(), [g.tobytes() for g in got], verdicts.tolist(), rc,
                f_out.cpu().numpy().tobytes(), f_sizes.cpu().tolist(), d_points.cpu().numpy().tobytes())

    shared = native.Codec(native.Plan(info))
    fresh = [native.Codec(native.Plan(info)) for _ in range(4)]
    a, b = run([shared] * 4), run(fresh)
    for c in [shared] + fresh:
        c.close()
    assert a == b
    b_out, b_sizes, got, verdicts, rc, f_out, f_sizes, points = a
    assert b_sizes == [18, 18] and b_out == lits[0] + b"\xa5" * 14 + lits[1] + b"\xa5" * 14
    assert rc == 0 and got == [w.tobytes() for w in want_points[ZSTD]] and verdicts == [p.size for p in payloads[ZSTD]]
    assert f_sizes == [40, 100] and f_out == texts[0] + b"\xa5" * 24 + texts[1] + b"\xa5" * 28
    assert points == b"".join(w.tobytes() for w in want_points[LZ4])
