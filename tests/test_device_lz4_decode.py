"""LZ4 blocks decoded on the device (cloudini_amd/csrc/lz4_decode.hip): cldn_hip_lz4_decompress, cldn_hip_decode_lz4 and the
host mirror's switch.

Expected values never come from the code under test: payloads are what went into liblz4 / oracle.lz4_model, verdicts come
from the strict rules of tests/lz4_block_rules.py (pinned one-sidedly against the system liblz4 on the CPU), points from
the compiled reference's decode of the reference's own LZ4 message."""

import numpy as np
import pytest

import lz4_block_rules as R
from cloudini_amd import synth
from cloudini_amd.schema import CompressionOption
from test_device_lz4 import GPU_CASES, _chunks

REJ = R.REJECTED


def _undamaged_blocks(oracle, n):
    """(label, block, payload) for every payload kind of size n: liblz4's block and the device model's (both parameter sets)."""
    rs = np.random.RandomState(n)
    for kind, payload in R.payload_kinds(rs, n):
        yield f"{kind}/{n}/liblz4", R.lz4_compress(payload), payload
        yield f"{kind}/{n}/model", oracle.lz4_model(payload).tobytes(), payload
        yield f"{kind}/{n}/model_fast", oracle.lz4_model(payload, 4096, 10, 512).tobytes(), payload


# ---- CPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.PAYLOAD_SIZES)
def test_rules_accept_every_undamaged_block(oracle, n):
    for label, block, payload in _undamaged_blocks(oracle, n):
        for cap in (len(payload), len(payload) + 64):
            assert R.decode(block, cap) == payload, (label, cap)
            assert R.lz4_decompress_safe(block, cap) == payload, (label, cap)


def test_rules_accept_the_largest_offset():
    payload = R.period_65535()
    block = R.lz4_compress(payload)
    assert len(block) < 70000                                                # (liblz4 did find the period)
    assert R.decode(block, len(payload)) == payload


def test_rules_accept_only_what_liblz4_accepts():
    """One-sided parity on the fixed-seed damaged corpus and the enumerated table: rules accept => liblz4 accepts, same bytes."""
    cases = R.damaged_corpus() + [(b, cap) for _n, b, cap, _ok in R.reject_table()]
    accepted = lenient = 0
    for block, cap in cases:
        got = R.decode(block, cap)
        if got is not None:
            accepted += 1
            assert R.lz4_decompress_safe(block, cap) == got, (block[:64].hex(), len(block), cap)
        elif R.lz4_decompress_safe(block, cap) is not None:
            lenient += 1
    print(f"{len(cases)} cases: {accepted} accepted by the rules, {lenient} more by liblz4 alone")
    assert accepted > len(cases) // 4 and len(cases) - accepted > len(cases) // 4   # (the corpus exercises both verdicts)
    for name, block, cap, ok in R.reject_table():
        assert (R.decode(block, cap) is not None) == ok, name


def test_structure_grid_blocks_are_valid_for_the_rules_and_for_liblz4():
    """Every block of the structural grid decodes to the payload its builder tracked, by the rules and by liblz4."""
    n = 0
    labels = set()
    for label, block, cap, payload in R.structure_grid():
        n += 1
        assert label not in labels, label
        labels.add(label)
        assert len(payload) <= cap
        assert R.decode(block, cap) == payload, label
        assert R.lz4_decompress_safe(block, cap) == payload, label
    assert 2000 < n < 5000, n


def test_damaged_grid_sample_shows_both_verdicts_and_liblz4_agrees():
    """R.damaged() on a fixed-seed sample of the grid: rules accept => liblz4 accepts, same bytes; both verdicts occur in
    at least a quarter of the cases each."""
    cases = R.damaged_grid_sample()
    accepted = lenient = 0
    for label, block, cap in cases:
        got = R.decode(block, cap)
        if got is not None:
            accepted += 1
            assert R.lz4_decompress_safe(block, cap) == got, label
        elif R.lz4_decompress_safe(block, cap) is not None:
            lenient += 1
    print(f"{len(cases)} damaged grid blocks: {accepted} accepted by the rules, {lenient} more by liblz4 alone")
    assert accepted > len(cases) // 4 and len(cases) - accepted > len(cases) // 4


def test_libraries_export_the_calls_and_the_switch_defaults_to_off():
    from cloudini_amd import api, native
    for name in ("cldn_hip_lz4_decompress", "cldn_hip_decode_lz4"):
        assert hasattr(native.lib(), name), name
    for name in ("cldn_amd_device_lz4_decode", "cldn_amd_set_device_lz4_decode"):
        assert hasattr(api.lib(), name), name
    assert api.device_lz4_decode() is False
    try:
        assert api.set_device_lz4_decode(True) is True and api.device_lz4_decode() is True
    finally:
        assert api.set_device_lz4_decode(False) is False
    assert api.device_lz4_decode() is False


# ---- GPU ---------------------------------------------------------------------------------------------------------------

GUARD = 64
FILL = 0xA5


def _codec():
    from cloudini_amd import native
    info, _ = synth.lidar_xyzi(10)
    return native.Codec(native.Plan(info))


def _run_device(codec, cases, r_in=0, r_out=0):
    """cases: [(block, capacity)] through cldn_hip_lz4_decompress on DEVICE buffers with a guard span of 64 bytes in front of
    and behind every output span (a guard is the span of a one-byte block 00: it decodes to nothing). Input and output start
    r_in / r_out bytes behind a 256-byte boundary. Returns (sizes, [span bytes], raised) after checking every guard."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    blocks, caps = [], []
    for block, cap in cases:
        blocks += [b"\x00", bytes(block)]
        caps += [GUARD, int(cap)]
    blocks.append(b"\x00")
    caps.append(GUARD)
    bo = np.zeros(len(blocks) + 1, dtype=np.uint64)
    bo[1:] = np.cumsum([len(b) for b in blocks])
    oo = np.zeros(len(blocks) + 1, dtype=np.uint64)
    oo[1:] = np.cumsum(caps)
    data = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    d_in = torch.zeros(256 + data.size + 256, dtype=torch.uint8, device=dev)
    base_in = (-d_in.data_ptr()) % 256 + r_in
    d_in[base_in:base_in + data.size] = torch.from_numpy(data.copy()).to(dev)
    total = int(oo[-1])
    d_out = torch.full((512 + total + 512,), FILL, dtype=torch.uint8, device=dev)
    base_out = (-d_out.data_ptr()) % 256 + 256 + r_out
    d_sizes = torch.full((len(blocks),), 0x77777777, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.lz4_decompress_device(d_in.data_ptr() + base_in, bo, d_out.data_ptr() + base_out, oo, d_sizes.data_ptr())
    raised = False
    try:
        codec.status()
    except native.CloudiniHipError as e:
        assert e.code == -6
        raised = True
    out = d_out.cpu().numpy()
    sizes = d_sizes.cpu().numpy().view(np.uint32)
    assert np.all(out[:base_out] == FILL) and np.all(out[base_out + total:] == FILL)   # nothing outside the batch's spans
    spans = []
    for k in range(len(blocks)):
        span = out[base_out + int(oo[k]):base_out + int(oo[k + 1])]
        if k % 2 == 0:
            assert sizes[k] == 0 and np.all(span == FILL), f"guard {k // 2} touched"
        else:
            spans.append(span)
    return sizes[1::2], spans, raised


def _check_against_rules(cases, sizes, spans, raised, labels=None):
    any_reject = False
    for k, (block, cap) in enumerate(cases):
        want = R.decode(block, cap)
        label = labels[k] if labels else (bytes(block[:48]).hex(), len(block), cap)
        if want is None:
            any_reject = True
            assert sizes[k] == REJ, label
        else:
            assert sizes[k] == len(want), label
            assert spans[k][: len(want)].tobytes() == want, label
            assert np.all(spans[k][len(want):] == FILL), label              # bytes behind the decoded ones keep their content
    assert raised == any_reject


@pytest.mark.gpu
def test_lz4_decompress_every_kind_and_size(oracle):
    codec = _codec()
    labels, cases, payloads = [], [], []
    for n in R.PAYLOAD_SIZES:
        for label, block, payload in _undamaged_blocks(oracle, n):
            labels.append(label)
            cases.append((block, len(payload)))
            payloads.append(payload)
    big = R.period_65535()
    labels.append("period65535")
    cases.append((R.lz4_compress(big), len(big) + 100))
    payloads.append(big)
    # DEVICE buffers
    sizes, spans, raised = _run_device(codec, cases)
    assert not raised
    for k, payload in enumerate(payloads):
        assert sizes[k] == len(payload), labels[k]
        assert spans[k][: len(payload)].tobytes() == payload, labels[k]
    # HOST buffers
    out, hsizes = codec.lz4_decompress_host([b for b, _ in cases], [c for _, c in cases])
    pos = 0
    for k, payload in enumerate(payloads):
        assert hsizes[k] == len(payload), labels[k]
        assert out[pos:pos + len(payload)].tobytes() == payload, labels[k]
        pos += cases[k][1]
    codec.close()


@pytest.mark.gpu
def test_lz4_decompress_at_every_address_residue(oracle):
    codec = _codec()
    rs = np.random.RandomState(5)
    payloads = [rs.randint(0, 256, 1000).astype(np.uint8).tobytes(), (bytes(range(7)) * 700)[:4096],
                rs.randint(0, 4, 70001).astype(np.uint8).tobytes(), bytes(40000), R.period_65535(70000)]
    cases = [(R.lz4_compress(p), len(p)) for p in payloads]
    cases += [(oracle.lz4_model(p).tobytes(), len(p) + 17) for p in payloads[:3]]
    want = payloads + payloads[:3]
    for r in range(16):
        sizes, spans, raised = _run_device(codec, cases, r_in=r, r_out=(7 * r + 3) % 16)
        assert not raised
        for k, p in enumerate(want):
            assert sizes[k] == len(p) and spans[k][: len(p)].tobytes() == p, (r, k)
    codec.close()


@pytest.mark.gpu
def test_lz4_decompress_mixed_batch_with_a_large_block():
    codec = _codec()
    rs = np.random.RandomState(9)
    big = (rs.randint(0, 256, 50000).astype(np.uint8).tobytes() + bytes(300000) + (b"abcdefghij" * 200000)[:1250000])
    assert len(big) == 1600000
    payloads = [b"", b"x", big, b"", b"y", bytes(100), b""]
    cases = [(R.lz4_compress(p), len(p)) for p in payloads]
    assert cases[0][0] == b"\x00"
    sizes, spans, raised = _run_device(codec, cases, r_in=3, r_out=9)
    assert not raised
    for k, p in enumerate(payloads):
        assert sizes[k] == len(p) and spans[k].tobytes() == p, k
    out, hsizes = codec.lz4_decompress_host([b for b, _ in cases], [c for _, c in cases])
    assert list(hsizes) == [len(p) for p in payloads] and out[: sum(len(p) for p in payloads)].tobytes() == b"".join(payloads)
    codec.close()


@pytest.mark.gpu
def test_lz4_decompress_reject_table():
    from cloudini_amd import native
    codec = _codec()
    table = R.reject_table()
    cases = [(b, cap) for _n, b, cap, _ok in table]
    names = [n for n, _b, _c, _ok in table]
    sizes, spans, raised = _run_device(codec, cases, r_in=1, r_out=5)
    for k, (name, _b, _cap, ok) in enumerate(table):
        assert (sizes[k] != REJ) == ok, name
    _check_against_rules(cases, sizes, spans, raised, names)
    # HOST buffers: the call itself reports the refused blocks, the others are decoded
    caps = [c for _, c in cases]
    out = np.full(max(1, sum(caps)), FILL, dtype=np.uint8)
    out, hsizes, rc = codec.lz4_decompress_host([b for b, _ in cases], caps, out=out)
    assert rc == -6 and "LZ4" in native.lib().cldn_hip_last_error().decode()
    pos = 0
    for k, (block, cap) in enumerate(cases):
        want = R.decode(block, cap)
        assert hsizes[k] == (REJ if want is None else len(want)), names[k]
        if want is not None:
            assert out[pos:pos + len(want)].tobytes() == want and np.all(out[pos + len(want):pos + cap] == FILL), names[k]
        pos += cap
    # a batch without a refused block reports nothing
    ok_cases = [c for c, (_n, _b, _c, ok) in zip(cases, table) if ok]
    sizes, spans, raised = _run_device(codec, ok_cases)
    assert not raised and REJ not in list(sizes)
    codec.close()


@pytest.mark.gpu
def test_lz4_decompress_damaged_corpus():
    codec = _codec()
    cases = R.damaged_corpus()
    sizes, spans, raised = _run_device(codec, cases, r_in=11, r_out=2)
    _check_against_rules(cases, sizes, spans, raised)
    codec.close()


def _grid_slices(grid, per_call=600):
    for i in range(0, len(grid), per_call):
        yield grid[i:i + per_call]


def _check_grid(codec, grid, r_in, r_out):
    for part in _grid_slices(grid):
        sizes, spans, raised = _run_device(codec, [(b, cap) for _l, b, cap, _p in part], r_in=r_in, r_out=r_out)
        assert not raised, (part[0][0], r_in, r_out)
        for k, (label, _b, cap, payload) in enumerate(part):
            assert sizes[k] == len(payload), (label, r_in, r_out, int(sizes[k]))
            got = spans[k][: len(payload)].tobytes()
            if got != payload:
                first = next(i for i in range(len(payload)) if got[i] != payload[i])
                raise AssertionError(f"{label} at residues ({r_in}, {r_out}): first wrong byte {first} of {len(payload)}")
            assert np.all(spans[k][len(payload):] == FILL), (label, r_in, r_out)


@pytest.mark.gpu
@pytest.mark.parametrize("r_in,r_out", [(0, 0), (5, 11)])
def test_lz4_decompress_structure_grid(r_in, r_out):
    """The whole structural grid on device buffers with guard spans: sizes and bytes are the builder's payload."""
    codec = _codec()
    _check_grid(codec, list(R.structure_grid()), r_in, r_out)
    codec.close()


@pytest.mark.gpu
def test_lz4_decompress_structure_grid_at_every_output_residue():
    """The ring index is output position + (dst & 15): a fixed-seed tenth of the grid at all 16 output residues."""
    grid = list(R.structure_grid())
    pick = np.random.RandomState(16).permutation(len(grid))[: len(grid) // 10]
    tenth = [grid[int(k)] for k in sorted(pick)]
    codec = _codec()
    for r in range(16):
        _check_grid(codec, tenth, (3 * r + 1) % 16, r)
    codec.close()


@pytest.mark.gpu
def test_lz4_decompress_structure_grid_from_host_buffers():
    codec = _codec()
    for part in _grid_slices(list(R.structure_grid())):
        caps = [cap for _l, _b, cap, _p in part]
        out = np.full(sum(caps), FILL, dtype=np.uint8)
        out, sizes, rc = codec.lz4_decompress_host([b for _l, b, _c, _p in part], caps, out=out)
        assert rc == 0
        pos = 0
        for k, (label, _b, cap, payload) in enumerate(part):
            assert sizes[k] == len(payload), label
            assert out[pos:pos + len(payload)].tobytes() == payload and np.all(out[pos + len(payload):pos + cap] == FILL), label
            pos += cap
    codec.close()


@pytest.mark.gpu
def test_lz4_decompress_damaged_grid_sample():
    codec = _codec()
    sample = R.damaged_grid_sample()
    for part in _grid_slices(sample, 800):
        cases = [(b, cap) for _l, b, cap in part]
        sizes, spans, raised = _run_device(codec, cases, r_in=7, r_out=13)
        _check_against_rules(cases, sizes, spans, raised, [l for l, _b, _c in part])
    codec.close()


def _lz4_body(reflib, info, data):
    """The reference's LZ4 message for the cloud, without its header, and the points the reference decodes from it."""
    linfo = info.copy(compression_opt=CompressionOption.LZ4)
    msg = reflib.encode(linfo, data)
    hdr = reflib.header(linfo)
    assert msg[: len(hdr)].tobytes() == hdr
    body = msg[len(hdr):].copy()
    return linfo, body, reflib.decode_noheader(linfo, body, fill=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_decode_lz4_equals_the_reference(reflib, oracle, name):
    import torch
    from cloudini_amd import native
    info, data = GPU_CASES[name]()
    n = data.size // info.point_step
    _linfo, body, want = _lz4_body(reflib, info, data)
    codec = native.Codec(native.Plan(info))
    # the stage-1 call on the stage-1 streams of the same batch: the routes the decoders take
    s1 = oracle.encode_stage1(info, data)
    assert np.array_equal(codec.decode_host([s1, s1], [n, n])[1], want)
    base_stats = codec.decode_stats()
    # the reference's blocks (liblz4), two clouds in the batch
    got = codec.decode_lz4_host([body, body], [n, n])
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    stats = codec.decode_stats()
    assert sum(stats) > 0
    for k in (2, 3):                                                         # no serial chunk where the stage-1 call shows none
        assert stats[k] == 0 or base_stats[k] != 0, (stats, base_stats)
    # our encoder's blocks, both parameter sets, device-resident from end to end
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(data.copy()).to(dev)
    for stage2 in (1, 2):
        codec.set_stage2(stage2)
        cap = codec.plan.stage2_bound(n, stage2)
        d_stream = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        codec.encode_device(d_in.data_ptr(), np.array([n], dtype=np.uint64), d_stream.data_ptr() + 5, cap, d_off.data_ptr())
        codec.status()
        offs = d_off.cpu().numpy().astype(np.uint64)
        codec.set_stage2(0)
        d_pts = torch.zeros(max(1, data.size), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        codec.decode_lz4_device(d_stream.data_ptr() + 5, offs, np.array([n], dtype=np.uint64), d_pts.data_ptr(), data.size)
        codec.status()
        assert np.array_equal(d_pts.cpu().numpy()[: data.size], want), stage2
    codec.close()


@pytest.mark.gpu
def test_decode_lz4_ragged_batch_with_empty_clouds(reflib):
    from cloudini_amd import native
    info, _ = synth.lidar_xyzi(10)
    codec = native.Codec(native.Plan(info))
    counts = [0, 5, 40000, 0, 32768, 33000, 0]
    bodies, wants = [], []
    for k, n in enumerate(counts):
        inf, data = synth.lidar_xyzi(n, seed=30 + k)
        _l, body, want = _lz4_body(reflib, inf, data)
        bodies.append(body)
        wants.append(want)
    got = codec.decode_lz4_host(bodies, counts)
    for k in range(len(counts)):
        assert np.array_equal(got[k], wants[k]), k
    assert codec.decode_lz4_host([bodies[0]], [0])[0].size == 0
    # a chain error is reported like the stage-1 call reports it
    with pytest.raises(native.CloudiniHipError) as e:
        codec.decode_lz4_host([bodies[2][:-1]], [counts[2]])
    assert e.value.code == -6
    codec.close()


def _break_first_match_offset(body: np.ndarray) -> np.ndarray:
    """The first match of the first chunk's block gets an offset beyond the start of the output."""
    b = bytearray(body.tobytes())
    p = 4
    token = b[p]
    p += 1
    ll = token >> 4
    if ll == 15:
        while True:
            s = b[p]
            p += 1
            ll += s
            if s != 255:
                break
    assert ll < 60000
    p += ll
    b[p] = 0xFF
    b[p + 1] = 0xFF
    return np.frombuffer(bytes(b), dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["xyzi_70k", "depth_rgba", "velodyne", "xyzi_3"])
def test_host_mirror_decodes_lz4_messages_on_the_device(reflib, name):
    from cloudini_amd import api
    info, data = GPU_CASES[name]()
    linfo, body, _want0 = _lz4_body(reflib, info, data)
    want = reflib.decode_noheader(linfo, body, fill=0x3C)
    dec = api.PointcloudDecoder()
    assert not api.device_lz4_decode()
    off = dec.decode(linfo, body, fill=0x3C)
    off_zero = dec.decode(linfo, body, output_is_zero=True)
    api.set_device_lz4_decode(True)
    try:
        on = dec.decode(linfo, body, fill=0x3C)
        on_zero = dec.decode(linfo, body, output_is_zero=True)
        on_threads = dec.decode(linfo.copy(use_threads=True), body, fill=0x3C)
    finally:
        api.set_device_lz4_decode(False)
    assert np.array_equal(off, want) and np.array_equal(on, want) and np.array_equal(on_threads, want)
    assert np.array_equal(on_zero, off_zero) and np.array_equal(on_zero, reflib.decode_noheader(linfo, body, fill=0))


@pytest.mark.gpu
def test_host_mirror_reports_a_damaged_block_on_both_routes(reflib):
    from cloudini_amd import api
    info, data = GPU_CASES["depth_rgba"]()
    linfo, body, _ = _lz4_body(reflib, info, data)
    bad = _break_first_match_offset(body)
    size = int.from_bytes(bad[:4].tobytes(), "little")
    block = bad[4:4 + size].tobytes()
    cap = 1 << 22
    assert R.decode(block, cap) is None and R.lz4_decompress_safe(block, cap) is None   # both refuse it
    dec = api.PointcloudDecoder()
    for on in (False, True):
        api.set_device_lz4_decode(on)
        try:
            with pytest.raises(RuntimeError, match="LZ4 decompression failed"):
                dec.decode(linfo, bad)
        finally:
            api.set_device_lz4_decode(False)
        assert np.array_equal(dec.decode(linfo, body), reflib.decode_noheader(linfo, body))   # and the decoder still works


@pytest.mark.gpu
def test_codec_alternates_lz4_decode_stage1_decode_and_encode(reflib, oracle):
    from cloudini_amd import native
    info, data = GPU_CASES["velodyne"]()
    n = data.size // info.point_step
    _l, body, want = _lz4_body(reflib, info, data)
    s1 = oracle.encode_stage1(info, data)
    codec = native.Codec(native.Plan(info))
    codec.set_stage2(1)
    first_blocks = codec.encode_host([data])[0][0]
    for _round in range(3):
        assert np.array_equal(codec.decode_lz4_host([body], [n])[0], want)
        codec.set_stage2(0)
        assert np.array_equal(codec.decode_host([s1], [n])[0], want)
        assert np.array_equal(codec.encode_host([data])[0][0], s1)
        codec.set_stage2(1)
        blocks = codec.encode_host([data])[0][0]
        assert np.array_equal(blocks, first_blocks)
        assert np.array_equal(codec.decode_lz4_host([blocks], [n])[0], want)
        out, sizes = codec.lz4_decompress_host([c.tobytes() for c in _chunks(blocks)], [c.size for c in _chunks(s1)])
        assert [int(x) for x in sizes] == [c.size for c in _chunks(s1)]
    codec.close()
