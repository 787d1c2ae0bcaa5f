"""cldn_hip_decode_zstd (ZSTD frames into per-chunk slots, then every stage-1 decoder reading the slots), the host mirror's
switch and cldn_hip_audit_streams with kind ZSTD.

Expected values: points from the oracle's stage-1 decoder; which bodies the device takes from tests/zstd_lit_rules.py at the
slot capacity (pinned against libzstd on the CPU, tests/test_zstd_lit_rules.py). Bodies are made three ways: the model
writer's frames (tests/zstd_lit_model.py) over the oracle's stage-1 chunks, the device writer's own output, and libzstd's."""
import numpy as np
import pytest

import cases
import zstd_decode_cases as K
import zstd_lit_model as M
import zstd_lit_rules as R
import zstd_payload_grid as G
from cloudini_amd.schema import CompressionOption, FieldType as F

FILL = 0xB7
ZSTD = 3
ERR_UNSUPPORTED, ERR_CORRUPT = -3, -6
FAMILIES = ["c2_xyzi", "c4_velodyne", "mixed_v5", "float_specials4"]
GRID = ["skewed_257", "skewed_131072", "three_byte_last_block", "full_block_then_another_run", "eight_blocks_mixed"]   # RAW1 / 4 / 5 / 32 / 32 (1 MiB)
_SIZE = {F.INT8: 1, F.UINT8: 1, F.INT16: 2, F.UINT16: 2, F.INT32: 4, F.UINT32: 4, F.FLOAT32: 4, F.FLOAT64: 8, F.INT64: 8, F.UINT64: 8}
_clouds = {}


def _cloud(name):
    if not _clouds:
        for nm, info, data in cases.encode_cases(small=True):
            if nm in FAMILIES:
                _clouds[nm] = (info, np.ascontiguousarray(data).view(np.uint8).reshape(-1))
        for nm in GRID:
            c = G.case(nm)
            _clouds[nm] = (G.schema(c.schema, c.clouds[0].size // G.STEPS[c.schema]), c.clouds[0])
    return _clouds[name]


def chunks_of(stream):
    s = np.ascontiguousarray(stream).view(np.uint8).reshape(-1)
    o, out = 0, []
    while o < s.size:
        n = int.from_bytes(s[o:o + 4].tobytes(), "little")
        out.append(s[o + 4:o + 4 + n])
        o += 4 + n
    return out


def body_of(s1, frame_of=M.frame):
    """[u32 size][ZSTD frame] per chunk of the framed stage-1 stream s1"""
    parts = []
    for p in chunks_of(s1):
        f = bytes(frame_of(p))
        parts += [len(f).to_bytes(4, "little"), f]
    return np.frombuffer(b"".join(parts), np.uint8) if parts else np.zeros(0, np.uint8)


def _filled(size):
    return np.full(max(1, size), FILL, dtype=np.uint8)


def _legs(oracle, plan, info, data, n, s1, body, want):
    import torch
    from cloudini_amd import native
    step = info.point_step
    dev = torch.device("cuda", 0)
    codec = native.Codec(plan)
    # a ragged batch of more than 8 clouds, an empty cloud and a one-point cloud among them
    rs = np.random.RandomState(n)
    cuts = sorted({0, n} | {int(c) for c in rs.randint(0, n + 1, 9)})
    parts = [data[a * step:b * step] for a, b in zip(cuts[:-1], cuts[1:])] + [data[:0], data[:step]]
    streams = [oracle.encode_stage1(info, q) for q in parts]
    npts = [len(q) // step for q in parts]
    got = codec.decode_zstd_host([body_of(s) for s in streams], npts, out=_filled(sum(npts) * step))
    for k, g in enumerate(got):
        assert np.array_equal(g, oracle.decode_stage1(info, streams[k], npts[k], fill=FILL)), ("batch cloud", k)
    # device-resident body and output at odd addresses, status through codec.status()
    mis_in, mis_out = 1 + n % 15, 1 + n // 7 % 15
    d_body = torch.zeros(body.size + 32, dtype=torch.uint8, device=dev)
    d_body[mis_in:mis_in + body.size] = torch.from_numpy(body.copy()).to(dev)
    d_pts = torch.full((data.size + 32,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.decode_zstd_device(d_body.data_ptr() + mis_in, np.array([0, body.size], dtype=np.uint64), np.array([n], dtype=np.uint64),
                             d_pts.data_ptr() + mis_out, data.size)
    codec.status()
    got = d_pts.cpu().numpy()
    assert np.array_equal(got[mis_out:mis_out + data.size], want[:data.size]), ("device resident", mis_in, mis_out)
    assert np.all(got[:mis_out] == FILL) and np.all(got[mis_out + data.size:] == FILL)
    codec.close()
    # CLDN_HIP_FILL_ZERO: every covered byte is the oracle's, every uncovered one the buffer's old byte or 0
    c2 = native.Codec(plan)
    c2.set_decode_fill(True)
    got = c2.decode_zstd_host([body], [n], out=_filled(data.size))[0].reshape(n, step)
    ref = want[:n * step].reshape(n, step)
    covered = np.zeros(step, dtype=bool)
    for f in info.fields:
        covered[f.offset:f.offset + _SIZE[F(int(f.type))]] = True
    assert np.array_equal(got[:, covered], ref[:, covered])
    assert np.all((got[:, ~covered] == FILL) | (got[:, ~covered] == 0))
    c2.close()
    # stale slots: large, then small, plain stage-1 calls in between
    n_small = max(1, n // 3)
    small = data[:n_small * step]
    s1_small = oracle.encode_stage1(info, small)
    want_small = oracle.decode_stage1(info, s1_small, n_small, fill=FILL)
    c3 = native.Codec(plan)
    for _round in range(2):
        assert np.array_equal(c3.decode_zstd_host([body], [n], out=_filled(data.size))[0], want), "stale slots: large"
        assert np.array_equal(c3.decode_host([s1_small], [n_small], out=_filled(small.size))[0], want_small)
        assert np.array_equal(c3.decode_zstd_host([body_of(s1_small)], [n_small], out=_filled(small.size))[0], want_small), "stale slots: small"
    c3.close()
    # the point kernel's launch shape: chained, 2 and 16 workgroups per chunk
    for split in (1, 2, 16):
        c4 = native.Codec(plan)
        assert c4.decode_split(split) == 0
        got = c4.decode_zstd_host([body, body], [n, n], out=_filled(2 * data.size))
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), ("split", split)
        c4.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES + GRID)
def test_decode_zstd_equals_the_oracle(oracle, name):
    from cloudini_amd import native
    info, data = _cloud(name)
    n = data.size // info.point_step
    s1 = oracle.encode_stage1(info, data)
    want = oracle.decode_stage1(info, s1, n, fill=FILL)
    plan = native.Plan(info)
    codec = native.Codec(plan)
    # the device writer's own stream, and the model writer's frames over the oracle's stage-1 chunks
    codec.set_stage2(ZSTD)
    own = codec.encode_host([data])[0][0]
    codec.set_stage2(0)
    for f in chunks_of(own):
        assert bytes(f[:5]) == bytes.fromhex("28b52ffda0")
    assert np.array_equal(codec.decode_zstd_host([own], [n], out=_filled(data.size))[0], want), "device-written frames"
    body = body_of(s1)
    assert np.array_equal(codec.decode_zstd_host([body], [n], out=_filled(data.size))[0], want), "model frames"
    codec.close()
    if name in FAMILIES or name == "three_byte_last_block":
        _legs(oracle, plan, info, data, n, s1, body, want)


def _expected_of(plan, body):
    """what the rules say about the frames of a body at the slot capacity: the worst verdict"""
    capacity = plan.stage1_bound(32768) + 60
    worst = R.OK
    for f in chunks_of(body):
        worst = R.worst(worst, R.decode(f.tobytes(), capacity)[0])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_decode_zstd_of_libzstd_bodies_is_points_or_unsupported(oracle, name):
    from cloudini_amd import native
    info, data = _cloud(name)
    n = data.size // info.point_step
    s1 = oracle.encode_stage1(info, data)
    want = oracle.decode_stage1(info, s1, n, fill=FILL)
    plan = native.Plan(info)
    codec = native.Codec(plan)
    seen = set()
    for params in (K.LEVEL1, K.SMALL_BLOCKS):
        body = body_of(s1, lambda p: K.libzstd_compress(p.tobytes(), params))
        expect = _expected_of(plan, body)
        seen.add(expect)
        assert expect != R.CORRUPT
        if expect == R.OK:
            assert np.array_equal(codec.decode_zstd_host([body], [n], out=_filled(data.size))[0], want)
        else:
            with pytest.raises(native.CloudiniHipError) as e:
                codec.decode_zstd_host([body], [n], out=_filled(data.size))
            assert e.value.code == ERR_UNSUPPORTED and "ZSTD frame carries sequences or options the device decoder does not take" in e.value.message
        assert np.array_equal(codec.decode_host([s1], [n], out=_filled(data.size))[0], want)      # the codec goes on
    print(name, sorted(seen))
    codec.close()


@pytest.mark.gpu
def test_decode_zstd_reports_refused_and_host_frames():
    """one chunk of a two-chunk body damaged: a flipped magic byte is refused ("ZSTD decompression failed"), a sequences byte of 1
    needs the host; both with HOST and with DEVICE outputs, and the codec decodes the intact body afterwards"""
    import torch
    from cloudini_amd import native
    from cloudini_amd import synth
    info, data = synth.lidar_xyzi(40000)
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    step = info.point_step
    n = data.size // step
    codec = native.Codec(native.Plan(info))
    codec.set_stage2(ZSTD)
    body = codec.encode_host([data])[0][0].copy()
    codec.set_stage2(0)
    frames = chunks_of(body)
    assert len(frames) == 2
    good = codec.decode_zstd_host([body], [n], out=_filled(data.size))[0].copy()
    second = 4 + frames[0].size + 4
    for at, delta, code, text in ((second, 1, ERR_CORRUPT, "ZSTD decompression failed"),
                                  (body.size - 1, 1, ERR_UNSUPPORTED, "ZSTD frame carries sequences or options the device decoder does not take")):
        bad = body.copy()
        bad[at] ^= delta
        assert R.decode(chunks_of(bad)[1].tobytes(), 1 << 24)[0] == (R.CORRUPT if code == ERR_CORRUPT else R.HOST)
        with pytest.raises(native.CloudiniHipError) as e:
            codec.decode_zstd_host([bad], [n], out=_filled(data.size))
        assert e.value.code == code and text in e.value.message
        d_body = torch.from_numpy(bad).to("cuda")
        d_pts = torch.full((data.size,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        codec.decode_zstd_device(d_body.data_ptr(), np.array([0, bad.size], dtype=np.uint64), np.array([n], dtype=np.uint64), d_pts.data_ptr(), data.size)
        with pytest.raises(native.CloudiniHipError) as e:
            codec.status()
        assert e.value.code == code and text in e.value.message
        assert np.array_equal(codec.decode_zstd_host([body], [n], out=_filled(data.size))[0], good)
    codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c4_velodyne", "mixed_v5"])
def test_host_mirror_decodes_the_same_points_with_the_switch_on_and_off(name):
    """device-ZSTD messages and libzstd messages, switch on and off: the points are identical in all four combinations"""
    from cloudini_amd import api
    info, data = _cloud(name)
    info = info.copy(compression_opt=CompressionOption.ZSTD)
    host_msg = api.PointcloudEncoder(info).encode(data)
    assert api.set_device_zstd(True) is True
    try:
        dev_msg = api.PointcloudEncoder(info).encode(data)
    finally:
        api.set_device_zstd(False)
    assert not np.array_equal(dev_msg, host_msg)
    want, _ = api.PointcloudDecoder().decode_stream(host_msg, fill=0x11)
    assert not api.device_zstd_decode()
    for msg in (dev_msg, host_msg):
        for on in (False, True):
            before = api.device_zstd_decode_count()
            api.set_device_zstd_decode(on)
            try:
                got, _ = api.PointcloudDecoder().decode_stream(msg, fill=0x11)
            finally:
                api.set_device_zstd_decode(False)
            assert np.array_equal(got, want), (name, on)
            # the device route is taken for the device-written message with the switch on, and only then (the fall-back is silent)
            assert api.device_zstd_decode_count() - before == (1 if on and msg is dev_msg else 0), (name, on, msg is dev_msg)


@pytest.mark.gpu
def test_audit_streams_with_kind_zstd_equals_the_plain_report():
    from cloudini_amd import native
    info, data = _cloud("c4_velodyne")
    codec = native.Codec(native.Plan(info))
    plain = codec.encode_host([data, data[:info.point_step * 1000]])[0]
    codec.set_stage2(ZSTD)
    framed = codec.encode_host([data, data[:info.point_step * 1000]])[0]
    codec.set_stage2(0)
    clouds = [data, data[:info.point_step * 1000]]
    want = codec.audit_streams_host(clouds, plain, 0)
    got = codec.audit_streams_host(clouds, framed, ZSTD)
    assert got.tobytes() == want.tobytes()
    codec.close()


# ---- chunk chain and frame damage through the decode call ---------------------------------------------------------------------

def _zero_frame(size: int) -> bytes:
    """a valid frame that decodes to exactly `size` zero bytes: RLE blocks of at most 128 KiB"""
    sizes = [M.BLOCK] * (size // M.BLOCK) + ([size % M.BLOCK] if size % M.BLOCK else [])
    return K.frame_header(size) + b"".join(M.block_header(k == len(sizes) - 1, M.RLE, s) + b"\x00" for k, s in enumerate(sizes))


def chain_table(oracle):
    """The enumerated rows of tests/test_decode_lz4_routes.py's chain_table re-made with ZSTD frames: (name, [bodies], [points per
    cloud]), one row per line of k_walk_chunks and per capacity rule, each next to its accepted neighbour."""
    import lz4_body as B
    from cloudini_amd import synth
    n = 2 * 32768 + 500
    info, data = synth.lidar_xyzi(n, seed=77)
    body = body_of(oracle.encode_stage1(info, data))
    frames = [f.tobytes() for f in chunks_of(body)]
    assert len(frames) == 3
    n2 = 900
    _info2, data2 = synth.lidar_xyzi(n2, seed=78)
    body2 = body_of(oracle.encode_stage1(info, data2))
    cap = B.capacity_of(oracle, info)
    at = [0, 4 + len(frames[0]), 8 + len(frames[0]) + len(frames[1])]

    def with_prefix(k, value):
        b = body.copy()
        b[at[k]:at[k] + 4] = np.frombuffer(int(value).to_bytes(4, "little"), dtype=np.uint8)
        return b

    empty = M.frame(b"")
    t = [("intact", [body], [n]), ("intact batch", [body, body2], [n, n2])]
    for k in range(3):
        t.append((f"prefix {k} is 0", [with_prefix(k, 0)], [n]))
        t.append((f"prefix {k} one less", [with_prefix(k, len(frames[k]) - 1)], [n]))
        t.append((f"prefix {k} one more", [with_prefix(k, len(frames[k]) + 1)], [n]))
        t.append((f"prefix {k} is 0xffffffff", [with_prefix(k, 0xFFFFFFFF)], [n]))
    t.append(("last prefix reaches the end exactly", [with_prefix(2, body.size - at[2] - 4)], [n]))
    t.append(("last prefix one past the end", [with_prefix(2, body.size - at[2] - 4 + 1)], [n]))
    t.append(("first prefix spans the whole body", [with_prefix(0, body.size - 4)], [n]))
    t.append(("first prefix one past the end", [with_prefix(0, body.size - 3)], [n]))
    for keep in (1, 2, 3, 4):
        t.append((f"last prefix cut to {keep} bytes", [body[:at[2] + keep]], [n]))
    t.append(("a chunk missing", [B.frame(frames[:2])], [n]))
    t.append(("a chunk missing, points of two chunks declared", [B.frame(frames[:2])], [65536]))
    t.append(("a chunk extra", [B.frame(frames + [frames[2]])], [n]))
    t.append(("a chunk extra, its points declared", [B.frame([frames[0], frames[1], frames[0], frames[2]])], [n + 32768]))
    t.append(("a chunk extra, empty frame", [B.frame(frames + [empty])], [n]))
    t.append(("no points declared, one chunk", [body2], [0]))
    t.append(("no points declared, no bytes", [body2[:0]], [0]))
    t.append(("points declared, no bytes", [body2[:0]], [n2]))
    for k in range(3):
        t.append((f"frame {k} is the empty frame", [B.frame(frames[:k] + [empty] + frames[k + 1:])], [n]))
        t.append((f"frame {k} is one byte", [B.frame(frames[:k] + [b"\x00"] + frames[k + 1:])], [n]))
        t.append((f"frame {k} has no bytes", [B.frame(frames[:k] + [b""] + frames[k + 1:])], [n]))
        t.append((f"frame {k} asks for the host", [B.frame(frames[:k] + [frames[k][:-1] + b"\x01"] + frames[k + 1:])], [n]))
    for size, what in ((cap - 1, "capacity - 1"), (cap, "exactly the capacity"), (cap + 1, "capacity + 1")):
        for k in (0, 2):
            t.append((f"frame {k} decodes to {what}", [B.frame(frames[:k] + [_zero_frame(size)] + frames[k + 1:])], [n]))
    t.append(("frames 0 and 1 swapped", [B.frame([frames[1], frames[0], frames[2]])], [n]))
    t.append(("frames 1 and 2 swapped", [B.frame([frames[0], frames[2], frames[1]])], [n]))
    t.append(("trailing byte behind the last frame", [np.concatenate([body, np.zeros(1, np.uint8)])], [n]))
    t.append(("trailing 4 bytes behind the last frame", [np.concatenate([body, np.zeros(4, np.uint8)])], [n]))
    t.append(("trailing bytes inside the last frame", [B.frame(frames[:2] + [frames[2] + b"\x00"])], [n]))
    bad2 = body2.copy()
    bad2[4] ^= 0xFF                                                        # (the magic of the first frame)
    t.append(("second cloud of a batch damaged", [body, bad2], [n, n2]))
    t.append(("second cloud of a batch cut", [body, body2[:-1]], [n, n2]))
    t.append(("first cloud of a batch cut", [body[:-1], body2], [n, n2]))
    t.append(("second cloud of a batch without bytes", [body, body2[:0]], [n, n2]))
    return info, t


REFUSED, NEEDS_HOST, STAGE1 = "ZSTD decompression failed", "ZSTD frame carries sequences or options the device decoder does not take", "stage-1"


_rules_seen = {}


def _rules(frame: bytes, cap: int):
    """R.decode, once per frame: most rows of the table share their frames"""
    if (frame, cap) not in _rules_seen:
        _rules_seen[(frame, cap)] = R.decode(frame, cap)
    return _rules_seen[(frame, cap)]


def chain_model(oracle, info, bodies, counts, fill):
    """The composite model: the chain walk of tests/lz4_body.py (k_walk_chunks), the rules at slot capacity, the oracle's stage-1
    decoder. -> ([points per cloud], None) or (None, (error code, text)); a refused frame outranks one that needs the host,
    which outranks a chain or stage-1 error (the order of the call's status bits)."""
    import lz4_body as B
    cap = B.capacity_of(oracle, info)
    worst, points = 0, []
    for body, n in zip(bodies, counts):
        frames = B.walk(body, n)
        if frames is None:
            worst = max(worst, 1)
            continue
        got = [_rules(f, cap) for f in frames]
        if any(v == R.CORRUPT for v, _p in got):
            worst = max(worst, 3)
        elif any(v == R.HOST for v, _p in got):
            worst = max(worst, 2)
        else:
            try:
                points.append(oracle.decode_stage1(info, B.frame([p for _v, p in got]), n, fill=fill))
            except Exception:
                worst = max(worst, 1)
    if worst:
        return None, {1: (ERR_CORRUPT, STAGE1), 2: (ERR_UNSUPPORTED, NEEDS_HOST), 3: (ERR_CORRUPT, REFUSED)}[worst]
    return points, None


@pytest.mark.gpu
def test_chain_table_decodes_like_the_model(oracle):
    from cloudini_amd import native
    info, table = chain_table(oracle)
    codec = native.Codec(native.Plan(info))
    seen = set()
    for name, bodies, counts in table:
        want, err = chain_model(oracle, info, bodies, counts, FILL)
        out = _filled(sum(counts) * info.point_step)
        if want is None:
            seen.add(err[1])
            with pytest.raises(native.CloudiniHipError) as e:
                codec.decode_zstd_host(bodies, counts, out=out)
            assert e.value.code == err[0] and err[1] in e.value.message, (name, e.value.message)
            assert (REFUSED in e.value.message, NEEDS_HOST in e.value.message) == (err[1] == REFUSED, err[1] == NEEDS_HOST), name
        else:
            seen.add("accepted")
            got = codec.decode_zstd_host(bodies, counts, out=out)
            for k, w in enumerate(want):
                assert np.array_equal(got[k], w), (name, "cloud", k)
    assert seen == {"accepted", REFUSED, NEEDS_HOST, STAGE1}
    codec.close()
