"""cldn_hip_decode_zstd on libzstd-compressed bodies (frames WITH sequences, cldn_hip_codec_set_zstd_sequences), the host
mirror's second switch and cldn_hip_audit_streams with kind ZSTD on such bodies.

Expected values: points from the oracle's stage-1 decoder; which bodies the device takes from tests/zstd_seq_rules.py at the
slot capacity (pinned against libzstd on the CPU, tests/test_zstd_seq_rules.py)."""
import numpy as np
import pytest

import zstd_decode_cases as K
import zstd_seq_rules as S
from cloudini_amd.schema import CompressionOption, FieldType as F
from test_decode_zstd_routes import _SIZE, ERR_CORRUPT, ERR_UNSUPPORTED, FAMILIES, FILL, ZSTD, _cloud, _filled, body_of, chunks_of


LEVEL3 = ((K.C_LEVEL, 3),)       # (level 1 leaves the chunks of c2_xyzi literal-only here; level 3 finds matches in every family)


def _lib_body(s1, params=LEVEL3):
    return body_of(s1, lambda p: K.libzstd_compress(p.tobytes(), params))


def _codec(plan):
    from cloudini_amd import native
    codec = native.Codec(plan)
    codec.set_zstd_sequences(True)
    return codec


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_decode_zstd_of_libzstd_bodies_equals_the_oracle(oracle, name):
    import torch
    from cloudini_amd import native
    info, data = _cloud(name)
    step = info.point_step
    n = data.size // step
    s1 = oracle.encode_stage1(info, data)
    want = oracle.decode_stage1(info, s1, n, fill=FILL)
    plan = native.Plan(info)
    capacity = plan.stage1_bound(32768) + 60
    body = _lib_body(s1)
    verdicts = [S.decode_trace(f.tobytes(), capacity) for f in chunks_of(body)]
    assert all(v[0] == S.OK for v in verdicts) and any(v[2]["has_seq"] for v in verdicts), name
    # switch off: the call reports what it always reported
    plain = native.Codec(plan)
    with pytest.raises(native.CloudiniHipError) as e:
        plain.decode_zstd_host([body], [n], out=_filled(data.size))
    assert e.value.code == ERR_UNSUPPORTED and "ZSTD frame carries sequences or options the device decoder does not take" in e.value.message
    plain.close()
    codec = _codec(plan)
    assert np.array_equal(codec.decode_zstd_host([body], [n], out=_filled(data.size))[0], want), "level 3"
    assert np.array_equal(codec.decode_zstd_host([_lib_body(s1, K.LEVEL1)], [n], out=_filled(data.size))[0], want), "level 1"
    # a ragged batch of more than 8 clouds, an empty cloud and a one-point cloud among them
    rs = np.random.RandomState(n)
    cuts = sorted({0, n} | {int(c) for c in rs.randint(0, n + 1, 9)})
    parts = [data[a * step:b * step] for a, b in zip(cuts[:-1], cuts[1:])] + [data[:0], data[:step]]
    streams = [oracle.encode_stage1(info, q) for q in parts]
    npts = [len(q) // step for q in parts]
    got = codec.decode_zstd_host([_lib_body(s) for s in streams], npts, out=_filled(sum(npts) * step))
    for k, g in enumerate(got):
        assert np.array_equal(g, oracle.decode_stage1(info, streams[k], npts[k], fill=FILL)), ("batch cloud", k)
    # device-resident body and output at odd addresses, status through codec.status()
    dev = torch.device("cuda", 0)
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
    c2 = _codec(plan)
    c2.set_decode_fill(True)
    got = c2.decode_zstd_host([body], [n], out=_filled(data.size))[0].reshape(n, step)
    ref = want[:n * step].reshape(n, step)
    covered = np.zeros(step, dtype=bool)
    for f in info.fields:
        covered[f.offset:f.offset + _SIZE[F(int(f.type))]] = True
    assert np.array_equal(got[:, covered], ref[:, covered])
    assert np.all((got[:, ~covered] == FILL) | (got[:, ~covered] == 0))
    c2.close()
    # stale slots and scratch: large, then small, plain stage-1 calls in between
    n_small = max(1, n // 3)
    small = data[:n_small * step]
    s1_small = oracle.encode_stage1(info, small)
    want_small = oracle.decode_stage1(info, s1_small, n_small, fill=FILL)
    c3 = _codec(plan)
    for _round in range(2):
        assert np.array_equal(c3.decode_zstd_host([body], [n], out=_filled(data.size))[0], want), "stale slots: large"
        assert np.array_equal(c3.decode_host([s1_small], [n_small], out=_filled(small.size))[0], want_small)
        assert np.array_equal(c3.decode_zstd_host([_lib_body(s1_small)], [n_small], out=_filled(small.size))[0], want_small), "stale slots: small"
    c3.close()
    # the point kernel's launch shape: chained, 2 and 16 workgroups per chunk
    for split in (1, 2, 16):
        c4 = _codec(plan)
        assert c4.decode_split(split) == 0
        got = c4.decode_zstd_host([body, body], [n, n], out=_filled(2 * data.size))
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), ("split", split)
        c4.close()


@pytest.mark.gpu
def test_a_refused_frame_in_mid_batch_gives_the_error_text(oracle):
    from cloudini_amd import native
    info, data = _cloud("c2_xyzi")
    n = data.size // info.point_step
    s1 = oracle.encode_stage1(info, data)
    plan = native.Plan(info)
    capacity = plan.stage1_bound(32768) + 60
    body = _lib_body(s1)
    frames = chunks_of(body)
    assert len(frames) >= 3
    codec = _codec(plan)
    good = codec.decode_zstd_host([body], [n], out=_filled(data.size))[0].copy()
    second = 4 + frames[0].size + 4
    for at, code, text in ((second, ERR_CORRUPT, "ZSTD decompression failed"),                     # the magic number
                           (second + 4, ERR_UNSUPPORTED, "ZSTD frame carries sequences or options the device decoder does not take")):
        bad = body.copy()
        bad[at] ^= 4                                                                                # (+4: the checksum flag)
        assert S.decode(chunks_of(bad)[1].tobytes(), capacity)[0] == (S.CORRUPT if code == ERR_CORRUPT else S.HOST)
        with pytest.raises(native.CloudiniHipError) as e:
            codec.decode_zstd_host([bad], [n], out=_filled(data.size))
        assert e.value.code == code and text in e.value.message
        assert np.array_equal(codec.decode_zstd_host([body], [n], out=_filled(data.size))[0], good)
    codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("damage", ["size_word", "cut_short"])
def test_damaged_chunk_framing_in_mid_batch_is_refused_and_the_neighbours_decode(oracle, damage):
    """The [u32 size] chain of ONE cloud of a batch is damaged (its first size word beyond the body, or the body cut short in a
    frame): every chunk of that cloud has no valid span, so the walk has no frame for it -- and the execution must find that
    written, whatever an earlier call of another shape left in the codec's workspace. The call reports CORRUPT, the clouds on
    both sides decode."""
    import torch
    from cloudini_amd import native
    info, data = _cloud("c4_velodyne")
    step = info.point_step
    n = data.size // step
    s1 = oracle.encode_stage1(info, data)
    want = oracle.decode_stage1(info, s1, n, fill=FILL)
    body = _lib_body(s1)
    assert len(chunks_of(body)) >= 3
    codec = _codec(native.Plan(info))
    # calls of other shapes first: one cloud, then five, so the workspace holds another layout's words
    assert np.array_equal(codec.decode_zstd_host([body], [n], out=_filled(data.size))[0], want)
    got = codec.decode_zstd_host([body] * 5, [n] * 5, out=_filled(5 * data.size))
    assert all(np.array_equal(g, want) for g in got)
    bad = body.copy()
    if damage == "size_word":
        bad[:4] = np.frombuffer((body.size + 100).to_bytes(4, "little"), np.uint8)
    else:
        bad = bad[:bad.size - 7].copy()
    bodies = [body, bad, body]
    offs = np.zeros(4, dtype=np.uint64)
    offs[1:] = np.cumsum([b.size for b in bodies])
    dev = torch.device("cuda", 0)
    d_body = torch.from_numpy(np.concatenate(bodies)).to(dev)
    d_pts = torch.full((3 * data.size,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.decode_zstd_device(d_body.data_ptr(), offs, np.array([n, n, n], dtype=np.uint64), d_pts.data_ptr(), 3 * data.size)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.status()
    assert e.value.code == ERR_CORRUPT, e.value.message
    got = d_pts.cpu().numpy()
    assert np.array_equal(got[:data.size], want[:data.size]), "the cloud in front"
    assert np.array_equal(got[2 * data.size:], want[:data.size]), "the cloud behind"
    # the codec goes on
    assert np.array_equal(codec.decode_zstd_host([body], [n], out=_filled(data.size))[0], want)
    codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c4_velodyne", "mixed_v5"])
def test_host_mirror_takes_libzstd_messages_only_with_both_switches(name):
    from cloudini_amd import api
    info, data = _cloud(name)
    info = info.copy(compression_opt=CompressionOption.ZSTD)
    msg = api.PointcloudEncoder(info).encode(data)
    want, _ = api.PointcloudDecoder().decode_stream(msg, fill=0x11)
    assert not api.device_zstd_decode() and not api.device_zstd_sequences()
    for decode_on in (False, True):
        for seq_on in (False, True):
            before = api.device_zstd_decode_count()
            api.set_device_zstd_decode(decode_on)
            api.set_device_zstd_sequences(seq_on)
            try:
                got, _ = api.PointcloudDecoder().decode_stream(msg, fill=0x11)
            finally:
                api.set_device_zstd_decode(False)
                api.set_device_zstd_sequences(False)
            assert np.array_equal(got, want), (name, decode_on, seq_on)
            assert api.device_zstd_decode_count() - before == (1 if decode_on and seq_on else 0), (name, decode_on, seq_on)


def test_host_mirror_exports_the_switch_and_it_defaults_to_off():
    from cloudini_amd import api
    for name in ("cldn_amd_device_zstd_sequences", "cldn_amd_set_device_zstd_sequences"):
        assert hasattr(api.lib(), name), name
    assert api.device_zstd_sequences() is False
    try:
        assert api.set_device_zstd_sequences(True) is True and api.device_zstd_sequences() is True
    finally:
        assert api.set_device_zstd_sequences(False) is False
    assert api.device_zstd_sequences() is False and api.device_zstd_decode() is False


@pytest.mark.gpu
def test_audit_streams_with_kind_zstd_on_libzstd_bodies_equals_the_plain_report(oracle):
    from cloudini_amd import native
    info, data = _cloud("c4_velodyne")
    codec = native.Codec(native.Plan(info))
    clouds = [data, data[:info.point_step * 1000]]
    plain = codec.encode_host(clouds)[0]
    framed = [_lib_body(s) for s in plain]
    want = codec.audit_streams_host(clouds, plain, 0)
    with pytest.raises(native.CloudiniHipError):
        codec.audit_streams_host(clouds, framed, ZSTD)
    codec.set_zstd_sequences(True)
    got = codec.audit_streams_host(clouds, framed, ZSTD)
    assert got.tobytes() == want.tobytes()
    codec.close()
