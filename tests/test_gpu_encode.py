"""GPU parity: the HIP stage-1 encoder (through the C ABI) against the CPU oracle, bit for bit."""
import os

import numpy as np
import pytest

from cloudini_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from cloudini_amd.schema import CompressionOption, EncodingInfo, EncodingOptions, FieldType, PointField

pytestmark = pytest.mark.gpu


def _first_diff(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if d.size else n


def check_encode(oracle, info, clouds):
    """Every encoder pipeline the schema allows (piece kernel + slots, generic kernel + slots) against the oracle."""
    from cloudini_amd import native
    plan = native.Plan(info)
    codec = native.Codec(plan)
    wants = [oracle.encode_stage1(info, cloud, return_modes=True) for cloud in clouds]
    streams = None
    taken_all = set()
    for mode in (2, 1):
        taken = codec.pipeline(mode)
        if taken in taken_all:   # the schema does not allow this pipeline: it falls back to one already checked
            continue
        taken_all.add(taken)
        streams, chunk_sizes, modes = codec.encode_host(clouds)
        tag = {1: "generic kernel + slots", 2: "piece kernel + slots"}[taken]
        pos = 0
        for k, cloud in enumerate(clouds):
            want, want_modes = wants[k]
            got = streams[k]
            assert len(got) == len(want), f"{tag} cloud {k}: size {len(got)} != {len(want)} (first diff at {_first_diff(got, want)})"
            assert np.array_equal(got, want), f"{tag} cloud {k}: first diff at byte {_first_diff(got, want)}"
            if plan.adaptive_fields:
                assert list(modes[k]) == list(want_modes), tag
            # chunk_sizes = the [u32 size] prefixes of the stream
            o = 0
            while o < len(want):
                size = int.from_bytes(bytes(want[o:o + 4]), "little")
                assert int(chunk_sizes[pos]) == size, f"{tag} cloud {k}: chunk size table"
                pos += 1
                o += 4 + size
    codec.close()
    return streams


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 32767, 32768, 32769, 70000])
def test_xyz_sizes(oracle, n):
    info, data = synth.lidar_xyz(n)
    check_encode(oracle, info, [data])


def test_xyz_uniform_worst_case(oracle):
    info, data = synth.uniform_xyz(100000)
    check_encode(oracle, info, [data])


def test_xyz_batch_ragged(oracle):
    clouds = []
    info = None
    for k, n in enumerate([5, 40000, 0, 32768, 1]):
        info, data = synth.lidar_xyz(n, seed=100 + k)
        clouds.append(data)
    check_encode(oracle, info, clouds)


def test_special_values(oracle):
    n = 5000
    rs = np.random.RandomState(3)
    pts = rs.uniform(-100, 100, size=(n, 3)).astype(np.float32)
    pts[rs.randint(0, n, 300), rs.randint(0, 3, 300)] = np.nan
    pts[rs.randint(0, n, 50), rs.randint(0, 3, 50)] = np.inf
    pts[rs.randint(0, n, 50), rs.randint(0, 3, 50)] = -np.inf
    pts[rs.randint(0, n, 50), rs.randint(0, 3, 50)] = 3e9
    pts[rs.randint(0, n, 50), rs.randint(0, 3, 50)] = -3e9
    pts[rs.randint(0, n, 50), rs.randint(0, 3, 50)] = 1e-42  # denormal
    pts[10:20] = np.round(pts[10:20]) + 0.5e-3  # exact half ticks at 1 mm
    info = synth.xyz_info(n)
    check_encode(oracle, info, [pts.view(np.uint8).reshape(-1)])


def test_xyzi_float4(oracle):
    n = 50000
    rs = np.random.RandomState(5)
    pts = rs.uniform(-30, 30, size=(n, 4)).astype(np.float32)
    info = EncodingInfo(fields=[PointField(c, 4 * i, FieldType.FLOAT32, 0.001) for i, c in enumerate("xyzi")],
                        width=n, height=1, point_step=16, encoding_opt=EncodingOptions.LOSSY,
                        compression_opt=CompressionOption.NONE)
    check_encode(oracle, info, [pts.view(np.uint8).reshape(-1)])


import cases  # noqa: E402

ALL = cases.encode_cases(small=False)


@pytest.mark.parametrize("name,info,data", ALL, ids=[c[0] for c in ALL])
def test_all_schema_families(oracle, name, info, data):
    check_encode(oracle, info, [data])


@pytest.mark.parametrize("ftype", [FieldType.UINT64, FieldType.INT64])
@pytest.mark.parametrize("off64,lanes", [(25, 4), (17, 3), (18, 3), (19, 3), (21, 4), (23, 4), (24, 4)])
def test_a_64_bit_integer_field_at_an_odd_offset_keeps_its_top_bytes(oracle, ftype, off64, lanes):
    """Round 6, fuzz seed 923696 (a range no earlier campaign had run): a UINT64 field at offset 25 behind four float lanes. The
    piece kernel takes such a field from the dwords it loaded for the point; for an 8-byte field at an offset that is no multiple of
    4 that is THREE dwords -- rounds 2-5 took two, and the field's top 1..3 bytes never reached its column (values of 2^40 and more
    came out truncated: a shorter, wrong DeltaVarint section). Every misalignment, both pipelines, large and small values,
    and the decoder on the way back."""
    from cloudini_amd import native
    n = 70_001
    rs = np.random.RandomState(off64 * 7 + lanes)
    fields = [(f"f{k}", 4 + 4 * k, FieldType.FLOAT32, 0.01) for k in range(lanes)]
    fields.append(("big", off64, ftype, None))
    step = off64 + 8 + 3
    cols = {f"f{k}": np.cumsum(rs.normal(0, 0.01, n)).astype(np.float32) for k in range(lanes)}
    big = rs.randint(0 if ftype == FieldType.UINT64 else -2**62, 2**62, n, dtype=np.int64)
    big[::7] = rs.randint(0, 100, big[::7].size)          # small values between the large ones
    cols["big"] = big.astype(np.uint64 if ftype == FieldType.UINT64 else np.int64)
    info = cases.make_info(fields, step, n)
    data = cases.pack(info, cols, n)
    streams = check_encode(oracle, info, [data])
    codec = native.Codec(native.Plan(info))
    out = np.full(data.size, 0xA5, dtype=np.uint8)
    got = codec.decode_host([streams[0]], [n], out=out)[0]
    assert np.array_equal(got, oracle.decode_stage1(info, streams[0], n, fill=0xA5))
    codec.close()


@pytest.mark.parametrize("lanes", [3, 4])
@pytest.mark.parametrize("ftype", [FieldType.UINT16, FieldType.INT32, FieldType.UINT32, FieldType.INT64, FieldType.UINT64])
def test_integer_fields_at_every_offset_around_the_loaded_window(oracle, lanes, ftype):
    """An enumeration next to the fuzz campaigns (round 6): the piece kernel loads up to eight dwords per point behind the first float
    lane and takes integer fields that lie inside them from registers, others from memory. One full-range integer field at EVERY
    byte offset from right behind the float lanes to beyond the window, for 2-, 4- and 8-byte types: the field's bytes must reach
    its section whole wherever it lies (inside, straddling the window's end, outside; aligned or not)."""
    from cloudini_amd import native
    n = 9000
    size = {FieldType.UINT16: 2, FieldType.INT32: 4, FieldType.UINT32: 4, FieldType.INT64: 8, FieldType.UINT64: 8}[ftype]
    npt = {FieldType.UINT16: np.uint16, FieldType.INT32: np.int32, FieldType.UINT32: np.uint32, FieldType.INT64: np.int64,
           FieldType.UINT64: np.uint64}[ftype]
    rs = np.random.RandomState(lanes * 100 + size)
    ii = np.iinfo(npt)
    for first in (0, 2):                       # the float lanes 4-byte aligned, or not
        for off in range(first + 4 * lanes, first + 42):
            fields = [(f"f{k}", first + 4 * k, FieldType.FLOAT32, 0.001) for k in range(lanes)] + [("v", off, ftype, None)]
            step = off + size + int(rs.randint(0, 4))
            cols = {f"f{k}": np.cumsum(rs.normal(0, 0.01, n)).astype(np.float32) for k in range(lanes)}
            cols["v"] = rs.randint(max(ii.min, -2**62), min(ii.max, 2**62), n, dtype=np.int64).astype(npt)
            info = cases.make_info(fields, step, n)
            data = cases.pack(info, cols, n)
            want = oracle.encode_stage1(info, data)
            codec = native.Codec(native.Plan(info))
            got, _sizes, _modes = codec.encode_host([data])
            assert np.array_equal(got[0], want), (lanes, int(ftype), first, off, step)
            out = np.full(data.size, 0x11, dtype=np.uint8)
            assert np.array_equal(codec.decode_host([want], [n], out=out)[0], oracle.decode_stage1(info, want, n, fill=0x11)), (lanes, int(ftype), first, off)
            codec.close()


@pytest.mark.parametrize("mis_in,mis_out", [(0, 1), (0, 2), (0, 8), (1, 0), (2, 3), (3, 5), (0, 4), (2, 12)])
def test_device_buffers_at_any_address(oracle, mis_in, mis_out):
    """Round 6 (found by the corner-case campaign's device-resident leg): `out` at a device address that is no multiple of 16 --
    k_finish laid its copy items out by the stream OFFSET, not by the address, and misplaced bytes. The BASELINE shapes with input,
    stream and decoded output at odd device addresses, batches of ragged clouds, outputs written in place by the kernels."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    for make in (lambda: synth.lidar_xyzi(70_001, seed=5), lambda: synth.lidar_xyz(40_000, seed=6), lambda: synth.velodyne_xyzir(50_000, seed=7),
                 lambda: synth.depthcam_xyzrgba(320, 200, seed=8)):
        info, data = make()
        step = info.point_step
        n = data.size // step
        cuts = [0, n // 3, n // 3, n - 1, n]                       # ragged clouds, one of them empty, one of one point
        parts = [data[a * step:b * step] for a, b in zip(cuts[:-1], cuts[1:])]
        wants = [oracle.encode_stage1(info, q) for q in parts]
        npts = np.array([len(q) // step for q in parts], dtype=np.uint64)
        plan = native.Plan(info)
        codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
        cap = int(sum(plan.stage1_bound(int(k)) for k in npts))
        d_in = torch.zeros(data.size + 16, dtype=torch.uint8, device=dev)
        d_in[mis_in:mis_in + data.size] = torch.from_numpy(data).to(dev)
        d_out = torch.zeros(cap + 32, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(len(parts) + 1, dtype=torch.int64, device=dev)
        n_chunks = int(sum((int(k) + 32767) // 32768 for k in npts))
        d_sizes = torch.zeros(max(1, n_chunks), dtype=torch.int32, device=dev)
        for _ in range(2):                                          # (the second call runs with the first one's hints)
            codec.encode_device(d_in.data_ptr() + mis_in, npts, d_out.data_ptr() + mis_out, cap, d_off.data_ptr(), d_sizes.data_ptr(), 0)
            codec.status()
            offs = d_off.cpu().numpy().astype(np.uint64)
            got = d_out[mis_out:mis_out + int(offs[-1])].cpu().numpy()
            assert [int(offs[k + 1] - offs[k]) for k in range(len(parts))] == [w.size for w in wants]
            assert np.array_equal(got, np.concatenate(wants)), (info.point_step, mis_in, mis_out)
        d_dec = torch.full((data.size + 16,), 0x42, dtype=torch.uint8, device=dev)
        codec.decode_device(d_out.data_ptr() + mis_out, offs, npts, d_dec.data_ptr() + mis_in, data.size, d_sizes.data_ptr())
        codec.status()
        want_dec = np.concatenate([oracle.decode_stage1(info, w, int(k), fill=0x42) for w, k in zip(wants, npts)])
        assert np.array_equal(d_dec[mis_in:mis_in + data.size].cpu().numpy(), want_dec), (info.point_step, mis_in, mis_out)
        codec.close()
    # the size arrays themselves at addresses the kernels cannot write in place (stream_offsets 4 bytes off an 8-byte boundary, chunk_sizes
    # 2 bytes off a 4-byte one): filled by a copy behind the kernels instead -- same values
    info, data = synth.lidar_xyzi(70_001, seed=5)
    n = data.size // info.point_step
    plan = native.Plan(info)
    codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    want = oracle.encode_stage1(info, data)
    d_in = torch.from_numpy(data).to(dev)
    d_out = torch.zeros(plan.stage1_bound(n), dtype=torch.uint8, device=dev)
    d_meta = torch.zeros(256, dtype=torch.uint8, device=dev)
    for off_mis, size_mis in ((4, 0), (0, 2), (4, 2), (0, 0)):
        d_meta.zero_()
        codec.encode_device(d_in.data_ptr(), np.array([n], dtype=np.uint64), d_out.data_ptr(), d_out.numel(), d_meta.data_ptr() + off_mis,
                            d_meta.data_ptr() + 64 + size_mis, 0)
        codec.status()
        meta = d_meta.cpu().numpy()
        offs = meta[off_mis:off_mis + 16].copy().view(np.uint64)
        sizes = meta[64 + size_mis:64 + size_mis + 12].copy().view(np.uint32)
        assert int(offs[0]) == 0 and int(offs[1]) == want.size, (off_mis, size_mis, offs)
        assert int(sizes.astype(np.uint64).sum()) + 4 * 3 == want.size, (off_mis, size_mis, sizes)
        assert np.array_equal(d_out[:want.size].cpu().numpy(), want)
    codec.close()
    # LZ4 blocks on the device written at an odd address: the same bytes as at an aligned one (stage 2 of the same codec setting)
    info, data = synth.lidar_xyzi(70_001, seed=5)
    n = data.size // info.point_step
    plan = native.Plan(info)
    for level in (1, 2):
        codec = native.Codec(plan, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
        codec.set_stage2(level)
        cap = plan.stage2_bound(n, level)
        d_in = torch.zeros(data.size + 16, dtype=torch.uint8, device=dev)
        d_in[mis_in:mis_in + data.size] = torch.from_numpy(data).to(dev)
        outs = []
        for mo in (0, mis_out):
            d_out = torch.zeros(cap + 32, dtype=torch.uint8, device=dev)
            d_off = torch.zeros(2, dtype=torch.int64, device=dev)
            codec.encode_device(d_in.data_ptr() + mis_in, np.array([n], dtype=np.uint64), d_out.data_ptr() + mo, cap, d_off.data_ptr(), 0, 0)
            codec.status()
            total = int(d_off.cpu().numpy()[1])
            outs.append(d_out[mo:mo + total].cpu().numpy())
        assert outs[0].size > 0 and np.array_equal(outs[0], outs[1]), (level, mis_in, mis_out)
        codec.close()


def test_known_answer_vectors_gpu():
    from cloudini_amd import native
    for name, info, data, payload in cases.kat_vectors():
        codec = native.Codec(native.Plan(info))
        streams, chunk_sizes, _ = codec.encode_host([data])
        assert streams[0].tobytes()[4:] == payload, name
        assert list(chunk_sizes) == [len(payload)], name
        codec.close()


def test_reference_mode_bytes_gpu():
    from cloudini_amd import native
    for name, info, data, want in cases.reference_int_sequences():
        codec = native.Codec(native.Plan(info))
        streams, chunk_sizes, modes = codec.encode_host([data])
        s = streams[0]
        got = [int(s[4]), int(s[4 + 4 + int(chunk_sizes[0])])]
        if want is None:
            assert all(m != 3 for m in got), name
        else:
            assert got == want, name
        codec.close()


def test_batch_mixed_clouds_v5(oracle):
    clouds = []
    info = None
    for k, n in enumerate([100, 70000, 0, 4096, 4097, 32768, 33000]):
        info, data = synth.lidar_xyzi(n, seed=7 + k)
        clouds.append(data)
    check_encode(oracle, info, clouds)


def _check_both_ways(oracle, info, data):
    from cloudini_amd import native
    check_encode(oracle, info, [data])
    n = data.size // info.point_step
    want = oracle.encode_stage1(info, data)
    codec = native.Codec(native.Plan(info))
    out = np.full(max(1, data.size), 0xC3, dtype=np.uint8)
    got = codec.decode_host([want], [n], out=out)[0]
    assert np.array_equal(got, oracle.decode_stage1(info, want, n, fill=0xC3))
    codec.close()


def test_schemas_just_beyond_the_launch_argument_plan(oracle):
    """Round 5: the three schemas rounds 2-4 refused with CLDN_HIP_ERR_UNSUPPORTED -- a 1025-byte point, 65 per-point tokens
    (Gorilla-coded doubles), 65 adaptive integer fields -- take the WIDE route (stage1_wide.h) and match the oracle both ways.
    (Without a GPU cldn_hip_codec_create still fails with NO_DEVICE: there is no CPU fallback.)"""
    rs = np.random.RandomState(5)
    n = 5000
    x = np.cumsum(rs.normal(0, 0.01, n)).astype(np.float32)
    info = cases.make_info([("x", 0, FieldType.FLOAT32, 0.001)], 1025, n)  # point_step beyond kMaxPointStep
    _check_both_ways(oracle, info, cases.pack(info, {"x": x}, n))
    fields = [(f"g{k}", 8 * k, FieldType.FLOAT64, None) for k in range(65)]  # 65 per-point tokens, all Gorilla-coded
    info = cases.make_info(fields, 520, n)
    cols = {f"g{k}": (np.cumsum(rs.normal(0, 1e-3, n)) + k).astype(np.float64) for k in range(65)}
    _check_both_ways(oracle, info, cases.pack(info, cols, n))
    fields = [("x", 0, FieldType.FLOAT32, 0.001)] + [(f"u{k}", 4 + 2 * k, FieldType.UINT16, None) for k in range(65)]
    info = cases.make_info(fields, 134, n)  # 65 adaptive integer fields
    cols = {"x": x}
    for k in range(65):
        cols[f"u{k}"] = [(np.arange(n) % 64), rs.randint(0, 200, n) * 3, np.repeat(rs.randint(0, 9, n // 100 + 1), 100)[:n],
                         rs.randint(0, 65536, n)][k % 4].astype(np.uint16)
    _check_both_ways(oracle, info, cases.pack(info, cols, n))


def test_capacity_contract():
    from cloudini_amd import native
    import ctypes as C
    info, data = synth.lidar_xyz(1000)
    plan = native.Plan(info)
    codec = native.Codec(plan)
    npts = np.array([1000], dtype=np.uint64)
    out = np.zeros(100, dtype=np.uint8)
    rc = native.lib().cldn_hip_encode_stage1(codec._h, data.ctypes.data_as(C.c_void_p), 0,
                                             npts.ctypes.data_as(C.POINTER(C.c_uint64)), 1,
                                             out.ctypes.data_as(C.c_void_p), out.size, 0, None, None, None)
    assert rc == -2  # cloudini.cpp:531-534: "Output buffer too small for worst-case compressed size"
    codec.close()


# ---- one cloud encoded as chunk ranges with the modes of its head (cldn_hip_codec_force_modes) ------------------

def _split_encode(codec, info, data, world):
    from cloudini_amd import sharding
    step = info.point_step
    n = data.size // step
    modes = None
    if codec.plan.adaptive_fields:
        head = min(n, sharding.PROBE_POINTS)
        codec.force_modes(None)
        modes = codec.encode_host([data[: head * step]])[2][0]
        codec.force_modes(modes)
    parts = []
    for r in range(world):
        p0, cnt = sharding.shard_chunks(n, world, r)
        if cnt:
            parts.append(codec.encode_host([data[p0 * step:(p0 + cnt) * step]])[0][0])
    codec.force_modes(None)
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8), modes


@pytest.mark.parametrize("world", [2, 3, 8])
def test_chunk_range_parts_equal_whole_cloud(oracle, world):
    from cloudini_amd import native
    for info, data in (synth.lidar_xyzi(200_000, seed=9), synth.velodyne_xyzir(130048, seed=10),
                       synth.depthcam_xyzrgba(640, 400), synth.lidar_xyz(150_000, seed=11)):
        codec = native.Codec(native.Plan(info))
        got, modes = _split_encode(codec, info, data, world)
        want, want_modes = oracle.encode_stage1(info, data, return_modes=True)
        assert got.size == want.size and np.array_equal(got, want), f"first diff at {_first_diff(got, want)}"
        if modes is not None:
            assert list(modes) == list(want_modes)
        codec.close()


def test_forced_modes_override_the_probe(oracle):
    """Every forced mode must produce what the reference would write had it committed that mode: compare with the
    oracle's continued encoder, which takes the mode as given."""
    from cloudini_amd import native
    info, data = synth.lidar_xyzi(70_000, seed=12)
    codec = native.Codec(native.Plan(info))
    for mode in (0, 1, 2, 3):
        codec.force_modes([mode])
        got, _sizes, got_modes = codec.encode_host([data])
        want = oracle.encode_stage1_continued(info, data, [mode])
        assert np.array_equal(got[0], want), f"mode {mode}: first diff at {_first_diff(got[0], want)}"
        assert list(got_modes[0]) == [mode]
    codec.force_modes(None)
    got, _sizes, got_modes = codec.encode_host([data])
    assert np.array_equal(got[0], oracle.encode_stage1(info, data))
    with pytest.raises(native.CloudiniHipError):
        codec.force_modes([1, 2])       # one adaptive field in this schema
    with pytest.raises(native.CloudiniHipError):
        codec.force_modes([7])
    codec.close()


def test_mode_hints_never_change_the_bytes(oracle):
    """The section kernels launched for a call are picked from the modes an earlier call committed (a launch hint).
    A wrong hint may only cost time: same codec, clouds whose integer column commits a different mode every call."""
    from cloudini_amd import native
    rs = np.random.RandomState(77)
    n = 70_000
    base_info, base = synth.lidar_xyzi(n, seed=21)
    step = base_info.point_step
    variants = []
    for kind in ("palette", "delta", "drle", "rle", "palette", "rle", "delta"):
        data = base.copy().reshape(n, step)
        if kind == "palette":
            col = (rs.randint(0, 200, n) * 5).astype(np.uint16)
        elif kind == "delta":
            col = rs.randint(0, 65536, n).astype(np.uint16)
        elif kind == "drle":
            col = (np.arange(n) % 128).astype(np.uint16)
        else:
            col = np.repeat(rs.randint(0, 65536, n // 700 + 1), 700)[:n].astype(np.uint16)
        data[:, 12:14] = col.view(np.uint8).reshape(n, 2)
        variants.append((kind, data.reshape(-1)))
    codec = native.Codec(native.Plan(base_info))
    seen = set()
    for kind, data in variants:
        for _ in range(2):  # second pass runs with the hint of the first
            streams, _sizes, modes = codec.encode_host([data])
            want, want_modes = oracle.encode_stage1(base_info, data, return_modes=True)
            assert np.array_equal(streams[0], want), kind
            assert list(modes[0]) == list(want_modes)
        seen.add(int(want_modes[0]))
    assert seen == {0, 1, 2, 3}
    codec.close()


def test_one_codec_many_shapes_interleaved_with_decode(oracle):
    """Workspace and cached batch shapes: one codec, a random walk over batch shapes, encode and decode interleaved,
    forced modes toggled in between, every result checked."""
    from cloudini_amd import native
    rs = np.random.RandomState(123)
    info, _ = synth.lidar_xyzi(10, seed=0)
    pool = {n: synth.lidar_xyzi(n, seed=200 + n % 97)[1] for n in (0, 1, 63, 1000, 4096, 4097, 32768, 33000, 70000, 140000)}
    codec = native.Codec(native.Plan(info))
    step = info.point_step
    last_streams, last_counts = None, None
    for it in range(40):
        k = rs.randint(1, 6)
        sizes = [int(rs.choice(list(pool))) for _ in range(k)]
        clouds = [pool[n] for n in sizes]
        action = rs.randint(0, 4)
        if action == 3 and last_streams is not None:
            out = np.full(max(1, sum(last_counts) * step), 0x77, dtype=np.uint8)
            got = codec.decode_host(last_streams, last_counts, out=out)
            for s, cnt, g in zip(last_streams, last_counts, got):
                assert np.array_equal(g, oracle.decode_stage1(info, s, cnt, fill=0x77)), f"iteration {it}"
            continue
        if action == 2:
            codec.force_modes([int(rs.randint(0, 4))])
        streams, _cs, modes = codec.encode_host(clouds)
        for c, s, m in zip(clouds, streams, modes):
            if action == 2:
                want = oracle.encode_stage1_continued(info, c, [int(m[0])])
            else:
                want = oracle.encode_stage1(info, c)
            assert np.array_equal(s, want), f"iteration {it}, sizes {sizes}"
        codec.force_modes(None)
        last_streams, last_counts = streams, sizes
    codec.close()


def test_finish_timeout_is_retried_through_the_ticket_order():
    """k_finish waits for the records of the workgroups in front of it in dispatch order; when that wait runs out
    (ST_FINISH_TIMEOUT) a call with host outputs is redone once with the ticket counter (include/cloudini_hip.h,
    cldn_hip_codec_finish_retries). The debug call cldn_hip_debug_finish_timeout_once (outside the boundary) makes the first
    attempt report the timeout: the bytes must be those of an undisturbed call, one retry counted, and later calls of the
    codec go straight through tickets."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        from cloudini_amd import native, synth
        info, data = synth.lidar_xyzi(150000, seed=5)
        codec = native.Codec(native.Plan(info))
        if len(sys.argv) > 1:
            assert codec.finish_timeout_once() == 0
        a = codec.encode_host([data])[0][0]
        b = codec.encode_host([data])[0][0]
        print(codec.finish_retries(), int(np.array_equal(a, b)), a.size, int(a.view(np.uint8).sum()))
        codec.close()
    """ % ROOT)
    outs = []
    for extra in ([], ["hook"]):
        r = subprocess.run([sys.executable, "-c", code] + extra, capture_output=True, text=True, timeout=600, env=dict(os.environ))
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout.strip().splitlines()[-1].split())
    assert outs[0][0] == "0" and outs[1][0] == "1", outs   # one call redone, the second one takes tickets at once
    assert outs[0][1:] == outs[1][1:] and outs[0][1] == "1", outs
