"""The device ZSTD writer with matches (cldn_hip_codec_set_zstd_matches on top of CLDN_HIP_STAGE2_ZSTD;
cloudini_amd/csrc/zstd_seq_kernels.hip): frames whose blocks may hold sequences.

The kernels are held to byte equality with tests/zstd_match_model.py over the grid of tests/zstd_match_grid.py (that the
model's frames are valid ZSTD and that every case is what it was built for is held on the CPU, tests/test_zstd_match_model.py);
every frame the device wrote also goes through libzstd here. Full messages decode through the compiled reference, the host
mirror and this library's device decoder. With the switch off the bytes are tests/zstd_lit_model.py's."""
import ctypes as C

import numpy as np
import pytest

import cases
import sweep_model as S
import zstd_lit_model as L
import zstd_match_grid as G
import zstd_match_model as M
from cloudini_amd import synth
from cloudini_amd.schema import CompressionOption
from test_zstd_lit_model import zstd_decompress

pytestmark = pytest.mark.gpu

ZSTD = 3   # CLDN_HIP_STAGE2_ZSTD


def _chunks(stream: np.ndarray):
    out, o = [], 0
    while o < stream.size:
        size = int.from_bytes(stream[o:o + 4].tobytes(), "little")
        out.append(stream[o + 4:o + 4 + size])
        o += 4 + size
    assert o == stream.size
    return out


def _codec(info, on=True, **kw):
    from cloudini_amd import native
    codec = native.Codec(native.Plan(info), **kw)
    codec.set_stage2(ZSTD)
    codec.set_zstd_matches(on)
    return codec


def test_the_switch_is_a_switch():
    from cloudini_amd import native
    info, _ = synth.lidar_xyzi(10)
    codec = native.Codec(native.Plan(info))
    lib = native.lib()
    assert codec.zstd_matches() is False and lib.cldn_hip_codec_zstd_matches(None) == 0
    assert lib.cldn_hip_codec_set_zstd_matches(None, 1) != 0
    codec.set_zstd_matches(True)
    assert codec.zstd_matches() is True
    assert lib.cldn_hip_codec_set_stage2(codec._h, 4) == -1                       # not a stage-2 value
    plan = codec.plan
    assert plan.stage2_bound(40000, ZSTD) == native.Plan(info).stage2_bound(40000, ZSTD)
    codec.set_zstd_matches(False)
    assert codec.zstd_matches() is False
    codec.close()


@pytest.mark.parametrize("schema_name", sorted(G.STEPS))
def test_grid_frames_equal_the_model_and_decode(schema_name):
    """Every case of one raw-byte schema in one encode_host call, in file order and reversed (another source and destination
    alignment for every chunk): [u32][the model's frame] per chunk, chunk_sizes and the stream sizes to match, libzstd's verdict."""
    batch = G.batches()[schema_name]
    for c in batch:
        c.cond(G.traces(c))
    info = G.schema(schema_name)
    codec = _codec(info)
    for order in (batch, batch[::-1]):
        items = [(c, k) for c in order for k in range(len(c.clouds))]
        clouds = [c.clouds[k] for c, k in items]
        streams, chunk_sizes, _ = codec.encode_host(clouds)
        assert len(streams) == len(clouds)
        pos = 0
        for (c, k), cloud, stream in zip(items, clouds, streams):
            want = G.model(c)[k]
            frames = _chunks(stream)
            assert len(frames) == len(want), c.id
            assert stream.size == sum(4 + f.size for _p, f, _t in want), c.id      # the stream offsets are the model's
            for j, (frame, (raw, model, _trace)) in enumerate(zip(frames, want)):
                assert int(chunk_sizes[pos]) == frame.size == model.size, (c.id, j)
                pos += 1
                assert np.array_equal(frame, model), (c.id, j, int(np.nonzero(frame != model)[0][0]))
                assert zstd_decompress(frame.tobytes(), raw.size) == raw.tobytes(), (c.id, j)
        assert pos == len(chunk_sizes)
    codec.close()


@pytest.mark.parametrize("schema_name", ["RAW1", "RAW5"])
def test_frames_at_every_output_alignment(schema_name):
    """encode_device with `out` at 0, 1, 7 and 15 bytes from a 256-byte aligned buffer prefilled with 0xA5: the model's bytes at
    every offset (literal streams and the sequence bit stream are drained in 16-byte units between single bytes), nothing
    written in front of `out` or behind the reported total."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    batch = [c for c in map(G.case, G.ALIGNMENT_CASES + ["literals_four_streams", "match_ends_at_block_end"]) if c.schema == schema_name]
    assert batch
    info = G.schema(schema_name)
    step = G.STEPS[schema_name]
    codec = _codec(info, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    plan = codec.plan
    clouds = [c.clouds[0] for c in batch]
    npts = np.array([cl.size // step for cl in clouds], dtype=np.uint64)
    cap = int(sum(plan.stage2_bound(int(n), ZSTD) for n in npts))
    wants = []
    for c in batch:
        (_payload, frame, _trace), = G.model(c)[0]                               # one chunk each
        wants.append(np.concatenate([np.array([frame.size], dtype="<u4").view(np.uint8), frame]))
    want = np.concatenate(wants)
    want_offs = np.concatenate([[0], np.cumsum([w.size for w in wants])]).astype(np.uint64)
    d_in = torch.from_numpy(np.concatenate(clouds)).to(dev)
    front = 256
    for off in (0, 1, 7, 15):
        d_out = torch.full((front + 16 + cap + 256,), 0xA5, dtype=torch.uint8, device=dev)
        assert d_out.data_ptr() % 256 == 0
        d_off = torch.zeros(len(clouds) + 1, dtype=torch.int64, device=dev)
        d_sizes = torch.zeros(len(clouds), dtype=torch.int32, device=dev)
        codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr() + front + off, cap, d_off.data_ptr(), d_sizes.data_ptr(), 0)
        codec.synchronize()
        codec.status()
        host = d_out.cpu().numpy()
        offs = d_off.cpu().numpy().astype(np.uint64)
        assert np.array_equal(offs, want_offs), off
        assert [int(x) + 4 for x in d_sizes.cpu().numpy()] == [w.size for w in wants], off
        total = int(offs[-1])
        assert (host[:front + off] == 0xA5).all(), off
        assert (host[front + off + total:] == 0xA5).all(), off
        got = host[front + off:front + off + total]
        for c, a, b in zip(batch, want_offs[:-1], want_offs[1:]):
            assert np.array_equal(got[int(a):int(b)], want[int(a):int(b)]), (c.id, off)
    codec.close()


def _dds_batch():
    """the DDS layout (a ring field and a lossless float64 stamp), two clouds of two chunks and one without points"""
    info, data = cases.ouster_like(n=80000)
    step = info.point_step
    return info, [data[:45000 * step].copy(), np.zeros(0, np.uint8), data[45000 * step:].copy()]


def test_host_device_and_two_step_outputs_agree(oracle):
    """The same batch through HOST outputs, DEVICE outputs and the two-step host output (out = NULL, then fetch_output): the same
    bytes, which are the model's frames of the oracle's stage-1 payloads; smaller than the literal-only frames."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, clouds = _dds_batch()
    step = info.point_step
    codec = _codec(info)
    plan = codec.plan
    streams, chunk_sizes, modes = codec.encode_host(clouds)
    matched = 0
    for cloud, stream in zip(clouds, streams):
        payloads = _chunks(oracle.encode_stage1(info, cloud)) if cloud.size else []
        frames = _chunks(stream)
        assert len(frames) == len(payloads)
        for p, f in zip(payloads, frames):
            t = []
            assert f.tobytes() == M.frame_info(p, t)
            matched += sum(b["matched"] for b in t)
            assert f.size < len(L.frame(p))
    assert matched >= 4
    flat = np.concatenate(streams)
    npts = np.array([c.size // step for c in clouds], dtype=np.uint64)
    cap = int(sum(plan.stage2_bound(int(n), ZSTD) for n in npts))
    # DEVICE
    d_in = torch.from_numpy(np.concatenate(clouds)).to(dev)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(len(clouds) + 1, dtype=torch.int64, device=dev)
    d_sizes = torch.zeros(len(chunk_sizes), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr(), cap, d_off.data_ptr(), d_sizes.data_ptr(), 0)
    codec.synchronize()
    codec.status()
    offs = d_off.cpu().numpy()
    assert offs.tolist() == np.concatenate([[0], np.cumsum([s.size for s in streams])]).tolist()
    assert np.array_equal(d_out.cpu().numpy()[:flat.size], flat)
    assert np.array_equal(d_sizes.cpu().numpy().astype(np.uint32), chunk_sizes)
    # two-step HOST
    data = np.concatenate(clouds)
    offs2 = np.zeros(len(clouds) + 1, dtype=np.uint64)
    cs2 = np.zeros(len(chunk_sizes), dtype=np.uint32)
    native._check(native.lib().cldn_hip_encode_stage1(
        codec._h, data.ctypes.data_as(C.c_void_p), native.HOST, npts.ctypes.data_as(C.POINTER(C.c_uint64)), len(clouds),
        None, 0, native.HOST, offs2.ctypes.data_as(C.c_void_p), cs2.ctypes.data_as(C.c_void_p), None))
    assert offs2.tolist() == offs.tolist() and np.array_equal(cs2, chunk_sizes)
    out = np.zeros(int(offs2[-1]), dtype=np.uint8)
    native._check(native.lib().cldn_hip_codec_fetch_output(codec._h, out.ctypes.data_as(C.c_void_p), out.size))
    assert np.array_equal(out, flat)
    # the chunk-table call keeps refusing the mode
    with pytest.raises(native.CloudiniHipError) as e:
        codec.encode_chunks_device(d_in.data_ptr(), npts)
    assert e.value.code == -1
    codec.close()


def test_capacity_one_byte_short_of_the_produced_size():
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, clouds = _dds_batch()
    step = info.point_step
    codec = _codec(info)
    plan = codec.plan
    produced = sum(s.size for s in codec.encode_host(clouds)[0])
    npts = np.array([c.size // step for c in clouds], dtype=np.uint64)
    assert produced - 1 < int(sum(plan.stage2_bound(int(n), ZSTD) for n in npts))
    d_in = torch.from_numpy(np.concatenate(clouds)).to(dev)
    d_out = torch.full((256 + produced + 256,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr() + 256, produced - 1)
    assert e.value.code == -2                                                      # ST_OUT_OVERFLOW
    codec.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:256] == 0xA5).all() and (host[256 + produced - 1:] == 0xA5).all()
    codec.close()


FAMILIES = ["c2_xyzi", "c4_velodyne", "mixed_v5", "float_specials4", "ouster_like_gorilla"]
_family = {}


def _case(name):
    if not _family:
        for nm, info, data in cases.encode_cases(small=True):
            if nm in FAMILIES:
                keep = min(data.size // info.point_step, 50000)                     # two chunks at most
                _family[nm] = (info, data[:keep * info.point_step].copy())
    return _family[name]


@pytest.mark.parametrize("name", FAMILIES)
def test_messages_decode_through_the_reference_the_host_mirror_and_the_device(oracle, reflib, name):
    """Header with compression_opt ZSTD + the device's [u32][frame] chunks: the compiled reference and api.PointcloudDecoder
    return the points they return for the host-ZSTD message; cldn_hip_decode_zstd with the sequences switch returns them too,
    and its statistics show that the device took every chunk."""
    from cloudini_amd import api
    info, data = _case(name)
    info = info.copy(compression_opt=CompressionOption.ZSTD)
    step = info.point_step
    n = data.size // step
    codec = _codec(info)
    stream = codec.encode_host([data])[0][0]
    sized = info.copy(width=n, height=1)
    hdr = np.frombuffer(reflib.header(sized), np.uint8)
    host_msg = api.PointcloudEncoder(sized).encode(data)
    want, _ = reflib.decode(host_msg, data.size, fill=0x11)
    msg = np.concatenate([hdr, stream])
    got, _ = reflib.decode(msg, data.size, fill=0x11)
    assert np.array_equal(got, want)
    ours, _ = api.PointcloudDecoder().decode_stream(msg, fill=0x11)
    assert np.array_equal(ours, want)
    payloads = _chunks(oracle.encode_stage1(info, data))
    for p, f in zip(payloads, _chunks(stream)):
        assert f.tobytes() == M.frame_info(p)
    # the round trip on the device
    plain = codec.decode_host(_plain_streams(info, data), [n])[0]
    from cloudini_amd import native
    traces = []
    for p in payloads:
        M.frame_info(p, traces)
    if any(t["matched"] for t in traces):                                        # frames with sequences need the decoder's switch
        with pytest.raises(native.CloudiniHipError):
            codec.decode_zstd_host([stream], [n])
    codec.set_zstd_sequences(True)
    back = codec.decode_zstd_host([stream], [n])[0]
    assert np.array_equal(back, plain)
    stats = codec.decode_stats()
    assert stats[0] + stats[2] == len(payloads), stats                            # every chunk went through the device's point decoder
    codec.set_zstd_sequences(False)
    lit_size = sum(4 + len(L.frame(p)) for p in payloads)
    print(f"{name}: frames with matches / literal-only frames = {stream.size / lit_size:.4f}, / host ZSTD message = {msg.size / host_msg.size:.4f}")
    codec.close()


def _plain_streams(info, data):
    from cloudini_amd import native
    codec = native.Codec(native.Plan(info))
    streams, _cs, _m = codec.encode_host([data])
    codec.close()
    return streams


def test_last_encode_reports_equal_those_behind_a_plain_call():
    from cloudini_amd import native
    info, clouds = _dds_batch()
    ladders = S.default_ladders(info)
    codec = native.Codec(native.Plan(info))
    reports = {}
    for key, stage2, on in (("plain", 0, False), ("matches", ZSTD, True)):
        codec.set_stage2(stage2)
        codec.set_zstd_matches(on)
        streams, _cs, _m = codec.encode_host(clouds)
        reports[key] = (codec.audit_last_encode(), codec.audit_last_encode(), codec.stream_hist_last_encode(), streams)
    a0, _, h0, streams0 = reports["plain"]
    a1, a1_again, h1, streams1 = reports["matches"]
    assert a0.tobytes() == a1.tobytes() == a1_again.tobytes()                    # (the audit decodes the stage-1 streams behind the frames)
    want = np.stack([np.bincount(s, minlength=256) for s in streams0])           # the histogram is of those stage-1 streams too
    assert np.array_equal(h0.astype(np.int64), want) and np.array_equal(h1, h0)
    assert sum(s.size for s in streams1) < sum(s.size for s in streams0)
    codec.close()


def test_switch_off_writes_the_literal_only_frames_and_toggles_between_calls(oracle):
    """One codec, the switch toggled between calls: off -- the default, and again after it was on -- gives
    zstd_lit_model's frames, on gives zstd_match_model's. It has no effect on another stage 2."""
    from cloudini_amd import native
    info, clouds = _dds_batch()
    codec = native.Codec(native.Plan(info))
    codec.set_stage2(ZSTD)
    payloads = [_chunks(oracle.encode_stage1(info, c)) if c.size else [] for c in clouds]

    def frames_are(model):
        streams, _cs, _m = codec.encode_host(clouds)
        for ps, s in zip(payloads, streams):
            fs = _chunks(s)
            assert len(fs) == len(ps)
            for p, f in zip(ps, fs):
                assert f.tobytes() == model(p)
        return streams

    lit = frames_are(L.frame)                                                     # the default
    codec.set_zstd_matches(True)
    on = frames_are(M.frame_info)
    assert sum(s.size for s in on) < sum(s.size for s in lit)
    codec.set_zstd_matches(False)
    frames_are(L.frame)
    codec.set_zstd_matches(True)
    frames_are(M.frame_info)
    for other in (0, 1):                                                          # stage 1 only, LZ4: the switch changes nothing
        codec.set_stage2(other)
        a = codec.encode_host(clouds)[0]
        codec.set_zstd_matches(False)
        b = codec.encode_host(clouds)[0]
        codec.set_zstd_matches(True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    codec.close()


def test_host_mirror_writes_frames_with_matches_when_asked(reflib):
    from cloudini_amd import api
    info, data = cases.ouster_like(n=50000)
    info = info.copy(compression_opt=CompressionOption.ZSTD)
    ref_stream = reflib.encode(info, data)
    want, _ = reflib.decode(ref_stream, data.size, fill=0x11)
    assert api.device_zstd_matches() is False
    assert api.set_device_zstd_matches(True) is True                              # without set_device_zstd it changes nothing
    try:
        assert np.array_equal(api.PointcloudEncoder(info).encode(data), ref_stream)
        api.set_device_zstd(True)
        seq = api.PointcloudEncoder(info).encode(data)
        api.set_device_zstd_matches(False)
        lit = api.PointcloudEncoder(info).encode(data)
    finally:
        assert api.set_device_zstd_matches(False) is False
        api.set_device_zstd(False)
    assert seq.size < lit.size and not np.array_equal(seq, lit)                    # (the synthetic stamps repeat little: a gain of a percent)
    for msg in (seq, lit):
        got, _ = reflib.decode(msg, data.size, fill=0x11)
        assert np.array_equal(got, want)
    ours, _ = api.PointcloudDecoder().decode_stream(seq, fill=0x11)
    assert np.array_equal(ours, want)
    assert np.array_equal(api.PointcloudEncoder(info).encode(data), ref_stream)   # and off again
