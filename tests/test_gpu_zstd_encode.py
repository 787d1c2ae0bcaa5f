"""Stage 2 on the device for ZSTD (CLDN_HIP_STAGE2_ZSTD, cloudini_amd/csrc/zstd_kernels.hip): frames of literal-only blocks.

The kernels are held to byte equality with tests/zstd_lit_model.py over the payload grid of tests/zstd_payload_grid.py (that
the model's frames are valid ZSTD and that every case is what it was built for is held on the CPU, tests/test_zstd_lit_model.py);
every frame the device wrote also goes through libzstd here. Full messages -- header, then [u32][frame] per chunk -- decode
through the compiled reference and through this library's decoder to what the host-ZSTD message decodes to."""
import ctypes as C

import numpy as np
import pytest

import cases
import sweep_model as S
import zstd_lit_model as M
import zstd_payload_grid as G
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


def test_set_stage2_accepts_zstd():
    from cloudini_amd import native
    info, _ = synth.lidar_xyzi(10)
    codec = native.Codec(native.Plan(info))
    assert native.STAGE2_ZSTD == ZSTD
    assert native.lib().cldn_hip_codec_set_stage2(codec._h, ZSTD) == 0
    assert native.lib().cldn_hip_codec_set_stage2(codec._h, 4) == -1
    assert native.lib().cldn_hip_abi_version() == 1
    codec.close()


@pytest.mark.parametrize("schema_name", sorted(G.STEPS))
def test_grid_frames_equal_the_model_and_decode(oracle, schema_name):
    """Every case of one raw-byte schema in one encode_host call, in file order and reversed (another source and destination
    alignment for every chunk): [u32][the model's frame] per chunk, chunk_sizes and the stream sizes to match, libzstd's verdict."""
    from cloudini_amd import native
    batch = G.batches()[schema_name]
    info = G.schema(schema_name)
    codec = native.Codec(native.Plan(info))
    for order in (batch, batch[::-1]):
        items = [(c, k) for c in order for k in range(len(c.clouds))]
        clouds = [c.clouds[k] for c, k in items]
        codec.set_stage2(0)
        plain, plain_sizes, _ = codec.encode_host(clouds)
        codec.set_stage2(ZSTD)
        streams, chunk_sizes, _ = codec.encode_host(clouds)
        assert len(streams) == len(plain) == len(clouds)
        pos = 0
        for (c, k), cloud, s1, stream in zip(items, clouds, plain, streams):
            want = G.model(c)[k]
            payloads, frames = _chunks(s1), _chunks(stream)
            assert len(payloads) == len(frames) == len(want), c.id
            assert stream.size == sum(4 + f.size for _p, f, _t in want), c.id      # the stream offsets are the model's
            for j, (payload, frame, (raw, model, _trace)) in enumerate(zip(payloads, frames, want)):
                assert np.array_equal(payload, raw), (c.id, j)                     # the writer was handed the grid's bytes
                assert int(plain_sizes[pos]) == payload.size and int(chunk_sizes[pos]) == frame.size == model.size, (c.id, j)
                pos += 1
                assert np.array_equal(frame, model), (c.id, j, int(np.nonzero(frame != model)[0][0]))
                assert zstd_decompress(frame.tobytes(), raw.size) == raw.tobytes(), (c.id, j)
        assert pos == len(chunk_sizes) == len(plain_sizes)
    codec.close()


@pytest.mark.parametrize("schema_name", ["RAW1", "RAW5"])
def test_frames_at_every_output_alignment(schema_name):
    """encode_device with `out` at 0, 1, 7 and 15 bytes from a 256-byte aligned buffer prefilled with 0xA5: the model's bytes
    at every offset (the streams of a block are drained in 16-byte units between single bytes), nothing written in front of
    `out` or behind the reported total; stream_offsets and chunk_sizes as device arrays."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    batch = [c for c in map(G.case, G.ALIGNMENT_CASES) if c.schema == schema_name]
    assert batch
    info = G.schema(schema_name)
    step = G.STEPS[schema_name]
    plan = native.Plan(info)
    codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    codec.set_stage2(ZSTD)
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


def _velodyne_batch():
    info, data = synth.velodyne_xyzir(50000, seed=3)
    step = info.point_step
    return info, [data[:20000 * step].copy(), np.zeros(0, np.uint8), data[20000 * step:].copy()]


def test_host_device_and_two_step_outputs_agree(oracle):
    """The same batch through HOST outputs, DEVICE outputs and the two-step host output (out = NULL, then fetch_output): the same
    bytes, which are the model's frames of the oracle's stage-1 payloads."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, clouds = _velodyne_batch()
    step = info.point_step
    plan = native.Plan(info)
    codec = native.Codec(plan)
    codec.set_stage2(ZSTD)
    streams, chunk_sizes, modes = codec.encode_host(clouds)
    for cloud, stream in zip(clouds, streams):
        payloads = _chunks(oracle.encode_stage1(info, cloud)) if cloud.size else []
        frames = _chunks(stream)
        assert len(frames) == len(payloads)
        for p, f in zip(payloads, frames):
            assert f.tobytes() == M.frame(p)
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
    # the chunk-table call refuses the mode as it refuses LZ4
    with pytest.raises(native.CloudiniHipError) as e:
        codec.encode_chunks_device(d_in.data_ptr(), npts)
    assert e.value.code == -1
    codec.close()


def test_capacity_one_byte_short_of_the_produced_size():
    """`out` must offer the bound; a capacity of one byte less than what the call produces is refused with the capacity
    status and nothing is written: not inside `out`, not around it."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, clouds = _velodyne_batch()
    step = info.point_step
    plan = native.Plan(info)
    codec = native.Codec(plan)
    codec.set_stage2(ZSTD)
    produced = sum(s.size for s in codec.encode_host(clouds)[0])
    npts = np.array([c.size // step for c in clouds], dtype=np.uint64)
    assert produced - 1 < int(sum(plan.stage2_bound(int(n), ZSTD) for n in npts))
    d_in = torch.from_numpy(np.concatenate(clouds)).to(dev)
    d_out = torch.full((256 + produced + 256,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr() + 256, produced - 1)
    assert e.value.code == -2
    codec.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all()
    codec.close()


FAMILIES = ["c2_xyzi", "c4_velodyne", "mixed_v5", "float_specials4"]
_family = {}


def _case(name):
    if not _family:
        for nm, info, data in cases.encode_cases(small=True):
            if nm in FAMILIES:
                _family[nm] = (info, data)
    return _family[name]


@pytest.mark.parametrize("name", FAMILIES)
def test_messages_decode_through_the_reference_and_the_host_mirror(oracle, reflib, name):
    """Header with compression_opt ZSTD + the device's [u32][frame] chunks: the compiled reference and api.PointcloudDecoder
    return the points they return for the host-ZSTD message. Also with forced modes, and through the viz encode."""
    from cloudini_amd import api, native
    info, data = _case(name)
    info = info.copy(compression_opt=CompressionOption.ZSTD)
    step = info.point_step
    codec = native.Codec(native.Plan(info))

    def check(stream, points):
        sized = info.copy(width=points.size // step, height=1)                   # (the viz encode keeps fewer points)
        hdr = np.frombuffer(reflib.header(sized), np.uint8)
        host_msg = api.PointcloudEncoder(sized).encode(points)
        want, _ = reflib.decode(host_msg, points.size, fill=0x11)
        msg = np.concatenate([hdr, stream])
        for f in _chunks(stream):
            assert bytes(f[:5]) == bytes.fromhex("28b52ffda0")
        got, _ = reflib.decode(msg, points.size, fill=0x11)
        assert np.array_equal(got, want)
        ours, _ = api.PointcloudDecoder().decode_stream(msg, fill=0x11)
        assert np.array_equal(ours, want)
        return msg.size / host_msg.size

    codec.set_stage2(ZSTD)
    ratio = check(codec.encode_host([data])[0][0], data)
    print(f"{name}: device frames / host ZSTD message = {ratio:.4f}")
    if codec.plan.adaptive_fields:
        codec.force_modes([1] * codec.plan.adaptive_fields)
        check(codec.encode_host([data])[0][0], data)
        codec.force_modes(None)
    xyz = next((f.offset for f in info.fields if f.name == "x"), None)
    if xyz is not None and name != "float_specials4":
        streams, _cs, _m, kept = codec.encode_viz([data], xyz, 0.05)
        survivors = oracle.viz_preprocess(data, step, xyz, 0.05)
        assert int(kept[0]) == survivors.size // step
        check(streams[0], survivors)
    codec.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_bound_is_max_compressed_size(name):
    from cloudini_amd import api, native
    info, _ = _case(name)
    info = info.copy(compression_opt=CompressionOption.ZSTD)
    plan = native.Plan(info)
    for n in (1, 4096, 32768, 32769, 100000):
        assert plan.stage2_bound(n, ZSTD) == api.MaxCompressedSize(info, n, False), n
    n = 32768 * plan.max_point_bytes
    assert M.bound(n) == n + (n >> 8) + (((131072 - n) >> 11) if n < 131072 else 0)


def test_last_encode_reports_equal_those_behind_a_plain_call():
    from cloudini_amd import native
    info, clouds = _velodyne_batch()
    ladders = S.default_ladders(info)
    codec = native.Codec(native.Plan(info))
    reports = {}
    for stage2 in (0, ZSTD):
        codec.set_stage2(stage2)
        streams, _cs, _m = codec.encode_host(clouds)
        reports[stage2] = (codec.audit_last_encode(), codec.sweep_last_encode(ladders), codec.audit_last_encode(),
                           codec.stream_hist_last_encode(), streams)
    a0, s0, _, h0, streams0 = reports[0]
    a1, s1, a1_again, h1, streams1 = reports[ZSTD]
    assert a0.tobytes() == a1.tobytes() == a1_again.tobytes()                    # (the audit decodes the stage-1 streams behind the frames)
    assert S.same(s0, s1)
    want = np.stack([np.bincount(s, minlength=256) for s in streams0])           # the histogram is of those stage-1 streams too
    assert np.array_equal(h0.astype(np.int64), want) and np.array_equal(h1, h0)
    assert sum(s.size for s in streams1) < sum(s.size for s in streams0)
    codec.close()


def test_host_mirror_writes_device_frames_when_asked(reflib):
    from cloudini_amd import api
    info, data = synth.velodyne_xyzir(70000, seed=4)
    info = info.copy(compression_opt=CompressionOption.ZSTD)
    ref_stream = reflib.encode(info, data)
    want, _ = reflib.decode(ref_stream, data.size, fill=0x11)
    assert api.device_zstd() is False
    assert np.array_equal(api.PointcloudEncoder(info).encode(data), ref_stream)   # off: the reference's bytes
    assert api.set_device_zstd(True) is True and api.device_zstd() is True
    try:
        dev = api.PointcloudEncoder(info).encode(data)
    finally:
        assert api.set_device_zstd(False) is False
    hdr = reflib.header(info)
    assert dev[:len(hdr)].tobytes() == hdr and not np.array_equal(dev, ref_stream)
    got, _ = reflib.decode(dev, data.size, fill=0x11)
    assert np.array_equal(got, want)
    ours, _ = api.PointcloudDecoder().decode_stream(dev, fill=0x11)
    assert np.array_equal(ours, want)
    assert np.array_equal(api.PointcloudEncoder(info).encode(data), ref_stream)   # and off again
    info_lz4 = info.copy(compression_opt=CompressionOption.LZ4)                   # other compressions ignore the switch
    plain = api.PointcloudEncoder(info_lz4).encode(data)
    api.set_device_zstd(True)
    try:
        assert np.array_equal(api.PointcloudEncoder(info_lz4).encode(data), plain)
    finally:
        api.set_device_zstd(False)
