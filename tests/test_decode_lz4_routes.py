"""cldn_hip_decode_lz4 (LZ4 blocks into per-chunk slots, then every stage-1 decoder reading the slots) on every schema family,
on very wide schemas and on fresh fuzz seeds; damaged LZ4 bodies, fuzzed and enumerated.

Expected values: points from the oracle's stage-1 decoder, verdicts from the composite model of tests/lz4_body.py (chunk
chain + the strict block rules + the oracle). The CPU tests pin body and model against the compiled reference: the body is
the reference's byte for byte, and wherever the model accepts, the reference accepts with the same points."""
import numpy as np
import pytest

import lz4_block_rules as R
import lz4_body as B
from cloudini_amd.schema import FieldType as F

FILL = 0xB7
_SIZE = {F.INT8: 1, F.UINT8: 1, F.INT16: 2, F.UINT16: 2, F.INT32: 4, F.UINT32: 4, F.FLOAT32: 4, F.FLOAT64: 8,
         F.INT64: 8, F.UINT64: 8}
_IDS = B.cloud_ids()
_ID_NAMES = [f"{kind}-{key}" for kind, key in _IDS]
# the clouds whose bodies are damaged: every fourth family (all of them would mostly repeat the same chain damage on large
# clouds), every very wide one, every fuzz seed
_DAMAGE_IDS = [cid for k, cid in enumerate(_IDS) if cid[0] != "family" or k % 4 == 0]

_streams = {}
_verdicts = {}   # (cloud, damage kind) -> the model accepts: computed once per session


def _case(oracle, cid):
    """(info, data, number, n, stage-1 stream, LZ4 body), the two streams cached for the session."""
    info, data, number = B.cloud(*cid)
    n = data.size // info.point_step
    if cid not in _streams:
        s1 = oracle.encode_stage1(info, data)
        _streams[cid] = (s1, B.body_of(s1))
    s1, body = _streams[cid]
    return info, data, number, n, s1, body


def _ref_decode(reflib, info, body, n, fill):
    try:
        return reflib.decode_noheader(B.lz4_info(info).copy(width=n, height=1), np.ascontiguousarray(body, dtype=np.uint8), fill=fill)
    except Exception:
        return None


# ---- CPU: body and model against the reference --------------------------------------------------------------------------

def test_capacity_of_the_model_is_the_librarys(oracle):
    from cloudini_amd import native
    for cid in _IDS[::7]:
        info, _data, _k = B.cloud(*cid)
        assert B.capacity_of(oracle, info) == native.Plan(info).stage1_bound(32768) + 60, cid


def test_body_and_model_equal_the_reference(reflib, oracle):
    """For every cloud of the GPU tests: body_of(oracle's stream) is the body of the reference's LZ4 message, and the model
    decodes it to what the reference decodes."""
    small = []
    for cid in _IDS:
        info, data, _k, n, s1, body = _case(oracle, cid)
        linfo = B.lz4_info(info)
        msg = reflib.encode(linfo, data)
        hdr = reflib.header(linfo)
        assert msg[: len(hdr)].tobytes() == hdr, cid
        assert np.array_equal(msg[len(hdr):], body), cid
        cap = B.capacity_of(oracle, info)
        got = B.model(oracle, info, body, n, cap, FILL)
        assert got is not None, cid
        if B.reference_buffer_too_small(info, body, n, cap):                # (the reference refuses its own message: see there)
            small.append(cid)
            assert _ref_decode(reflib, info, body, n, FILL) is None, cid
            assert np.array_equal(got, oracle.decode_stage1(info, s1, n, fill=FILL)), cid
        else:
            assert np.array_equal(got, reflib.decode_noheader(linfo, body, fill=FILL)), cid
    print(f"{len(_IDS)} clouds; the reference's own buffer is too small for {len(small)}: {small}")
    assert len(small) * 20 < len(_IDS)


def _damaged_cases(oracle):
    for cid in _DAMAGE_IDS:
        info, _data, number, n, s1, body = _case(oracle, cid)
        if body.size < 8:
            continue
        for kind in B.DAMAGE_KINDS:
            yield cid, kind, info, n, body, B.damage(kind, number, s1, body)


def test_damaged_bodies_model_is_one_sided_against_the_reference(reflib, oracle):
    """Fuzzed damage: each verdict of the model occurs in at least 15 % of the cases (checked with the model alone); wherever
    the model accepts, the reference accepts with the same points."""
    total = accepted = ref_only = lz4_refusals = small = 0
    for cid, kind, info, n, _body, bad in _damaged_cases(oracle):
        cap = B.capacity_of(oracle, info)
        want = B.model(oracle, info, bad, n, cap, FILL)
        _verdicts[(cid, kind)] = want is not None
        total += 1
        ref = _ref_decode(reflib, info, bad, n, FILL)
        if want is not None:
            accepted += 1
            if B.reference_buffer_too_small(info, bad, n, cap):
                small += 1
                assert ref is None, (cid, kind)
            else:
                assert ref is not None and np.array_equal(ref, want), (cid, kind)
        else:
            ref_only += ref is not None
            lz4_refusals += B.refused_block(bad, n, cap)
    print(f"{total} damaged LZ4 bodies: the model accepts {accepted}, rejects {total - accepted} ({lz4_refusals} of them for a "
          f"refused block); the reference alone accepts {ref_only}; its own buffer is too small for {small} the model accepts")
    assert small * 20 < total
    assert accepted >= 0.15 * total and total - accepted >= 0.15 * total, (accepted, total)


def test_damaged_bodies_show_both_verdicts_by_the_model_alone(oracle):
    total = accepted = 0
    for cid, kind, info, n, _body, bad in _damaged_cases(oracle):
        total += 1
        if (cid, kind) not in _verdicts:
            _verdicts[(cid, kind)] = B.model(oracle, info, bad, n, B.capacity_of(oracle, info), FILL) is not None
        accepted += _verdicts[(cid, kind)]
    print(f"{total} damaged LZ4 bodies: the model accepts {accepted}")
    assert accepted >= 0.15 * total and total - accepted >= 0.15 * total, (accepted, total)


# ---- the enumerated chain table -----------------------------------------------------------------------------------------

def _block_of_size(size: int) -> bytes:
    """A valid block that decodes to exactly `size` zero bytes (size >= 13)."""
    return R._seq(b"\x00", 1, size - 1 - 12) + R._seq(bytes(12))


# the rows of chain_table() that are well formed by design: the accepted neighbours of the refused ones
CHAIN_ROWS_ACCEPTED = {"intact", "intact batch", "last prefix reaches the end exactly", "a chunk missing, points of two chunks declared",
                       "a chunk extra, its points declared", "no points declared, no bytes", "blocks 0 and 1 swapped"}


def chain_table(oracle):
    """(name, info, [bodies], [points per cloud]): one row per line of k_walk_chunks and per capacity rule, each next to its
    accepted neighbour. A three-chunk XYZI cloud and a one-chunk cloud of the same schema."""
    from cloudini_amd import synth
    n = 2 * 32768 + 500
    info, data = synth.lidar_xyzi(n, seed=77)
    s1 = oracle.encode_stage1(info, data)
    body = B.body_of(s1)
    blocks = [b.tobytes() for b in B.chunks_of(body)]
    assert len(blocks) == 3
    n2 = 900
    info2, data2 = synth.lidar_xyzi(n2, seed=78)
    body2 = B.body_of(oracle.encode_stage1(info2, data2))
    cap = B.capacity_of(oracle, info)
    at = [0, 4 + len(blocks[0]), 8 + len(blocks[0]) + len(blocks[1])]     # where the prefixes are

    def with_prefix(k, value):
        b = body.copy()
        b[at[k]:at[k] + 4] = np.frombuffer(int(value).to_bytes(4, "little"), dtype=np.uint8)
        return b

    t = [("intact", [body], [n]), ("intact batch", [body, body2], [n, n2])]
    for k in range(3):
        t.append((f"prefix {k} is 0", [with_prefix(k, 0)], [n]))
        t.append((f"prefix {k} one less", [with_prefix(k, len(blocks[k]) - 1)], [n]))
        t.append((f"prefix {k} one more", [with_prefix(k, len(blocks[k]) + 1)], [n]))
        t.append((f"prefix {k} is 0xffffffff", [with_prefix(k, 0xFFFFFFFF)], [n]))
    t.append(("last prefix reaches the end exactly", [with_prefix(2, body.size - at[2] - 4)], [n]))
    t.append(("last prefix one past the end", [with_prefix(2, body.size - at[2] - 4 + 1)], [n]))
    t.append(("first prefix spans the whole body", [with_prefix(0, body.size - 4)], [n]))
    t.append(("first prefix one past the end", [with_prefix(0, body.size - 3)], [n]))
    for keep in (1, 2, 3, 4):                                              # (4: the prefix is whole, its block is missing)
        t.append((f"last prefix cut to {keep} bytes", [body[: at[2] + keep]], [n]))
    t.append(("a chunk missing", [B.frame(blocks[:2])], [n]))
    t.append(("a chunk missing, points of two chunks declared", [B.frame(blocks[:2])], [65536]))
    t.append(("a chunk extra", [B.frame(blocks + [blocks[2]])], [n]))
    t.append(("a chunk extra, its points declared", [B.frame([blocks[0], blocks[1], blocks[0], blocks[2]])], [n + 32768]))
    t.append(("a chunk extra, empty block", [B.frame(blocks + [b"\x00"])], [n]))
    t.append(("no points declared, one chunk", [body2], [0]))
    t.append(("no points declared, no bytes", [body2[:0]], [0]))
    t.append(("points declared, no bytes", [body2[:0]], [n2]))
    for k in range(3):
        t.append((f"block {k} is 00", [B.frame(blocks[:k] + [b"\x00"] + blocks[k + 1:])], [n]))
        t.append((f"block {k} is empty", [B.frame(blocks[:k] + [b""] + blocks[k + 1:])], [n]))
    for size, what in ((cap - 1, "capacity - 1"), (cap, "exactly the capacity"), (cap + 1, "capacity + 1")):
        for k in (0, 2):
            t.append((f"block {k} decodes to {what}", [B.frame(blocks[:k] + [_block_of_size(size)] + blocks[k + 1:])], [n]))
    t.append(("blocks 0 and 1 swapped", [B.frame([blocks[1], blocks[0], blocks[2]])], [n]))
    t.append(("blocks 1 and 2 swapped", [B.frame([blocks[0], blocks[2], blocks[1]])], [n]))
    t.append(("trailing byte behind the last block", [np.concatenate([body, np.zeros(1, np.uint8)])], [n]))
    t.append(("trailing 4 bytes behind the last block", [np.concatenate([body, np.zeros(4, np.uint8)])], [n]))
    t.append(("trailing empty chunk behind the last block", [np.concatenate([body, np.array([1, 0, 0, 0, 0], np.uint8)])], [n]))
    t.append(("trailing bytes inside the last block", [B.frame(blocks[:2] + [blocks[2] + b"\x00"])], [n]))
    bad2 = body2.copy()
    bad2[4 + 1 + (bad2[4] >> 4)] ^= 0xFF                                   # (a byte behind the first token's literals)
    t.append(("second cloud of a batch damaged", [body, bad2], [n, n2]))
    t.append(("second cloud of a batch cut", [body, body2[:-1]], [n, n2]))
    t.append(("first cloud of a batch cut", [body[:-1], body2], [n, n2]))
    t.append(("second cloud of a batch without bytes", [body, body2[:0]], [n, n2]))
    return info, t


def _model_batch(oracle, info, bodies, counts, fill):
    """The batch's points, or None when any cloud of it is refused (the call fails as a whole)."""
    cap = B.capacity_of(oracle, info)
    res = [B.model(oracle, info, b, n, cap, fill) for b, n in zip(bodies, counts)]
    return None if any(r is None for r in res) else res


def test_chain_table_model_is_one_sided_against_the_reference(reflib, oracle):
    info, table = chain_table(oracle)
    accepted = ref_only = 0
    for name, bodies, counts in table:
        want = _model_batch(oracle, info, bodies, counts, FILL)
        assert (want is not None) == (name in CHAIN_ROWS_ACCEPTED), name
        refs = [_ref_decode(reflib, info, b, n, FILL) for b, n in zip(bodies, counts)]
        if want is not None:
            accepted += 1
            for w, r in zip(want, refs):
                assert r is not None and np.array_equal(r, w), name
        elif all(r is not None for r in refs):
            ref_only += 1
            print("the reference alone accepts:", name)
    print(f"{len(table)} rows of the chain table: the model accepts {accepted}, rejects {len(table) - accepted}; the reference "
          f"alone accepts {ref_only}")
    assert table[0][0] == "intact" and accepted == len(CHAIN_ROWS_ACCEPTED)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def _filled(size):
    return np.full(max(1, size), FILL, dtype=np.uint8)


def _no_new_serial_chunks(stats, base_stats):
    for k in (2, 3):                                                       # no serial chunk where the stage-1 call shows none
        assert stats[k] == 0 or base_stats[k] != 0, (stats, base_stats)


def _legs(oracle, codec, plan, info, data, n, s1, body, want, number, every_leg):
    """The legs behind the single-cloud host call, each for a fixed share of the clouds (all of them for the schema families)."""
    import torch
    from cloudini_amd import native
    step = info.point_step
    dev = torch.device("cuda", 0)
    if every_leg or number % 3 == 0:
        # a ragged BATCH of more than 8 clouds (the tables are uploaded, not passed as a kernel argument), an empty cloud and
        # a one-point cloud among them
        rs = np.random.RandomState(number)
        cuts = sorted({0, n} | {int(c) for c in rs.randint(0, n + 1, 9)})
        parts = [data[a * step:b * step] for a, b in zip(cuts[:-1], cuts[1:])] + [data[:0], data[:step]]
        while len(parts) < 10:
            parts.append(data[: (n // 2) * step])
        streams = [oracle.encode_stage1(info, q) for q in parts]
        npts = [len(q) // step for q in parts]
        got = codec.decode_lz4_host([B.body_of(s) for s in streams], npts, out=_filled(sum(npts) * step))
        for k, g in enumerate(got):
            assert np.array_equal(g, oracle.decode_stage1(info, streams[k], npts[k], fill=FILL)), (number, "batch cloud", k)
    if every_leg or number % 5 == 0:
        # DEVICE-RESIDENT body and output at odd addresses, status through codec.status()
        mis_in, mis_out = 1 + number // 5 % 15, 1 + number // 7 % 15
        d_body = torch.zeros(body.size + 32, dtype=torch.uint8, device=dev)
        d_body[mis_in:mis_in + body.size] = torch.from_numpy(body.copy()).to(dev)
        d_pts = torch.full((data.size + 32,), FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        codec.decode_lz4_device(d_body.data_ptr() + mis_in, np.array([0, body.size], dtype=np.uint64), np.array([n], dtype=np.uint64),
                                d_pts.data_ptr() + mis_out, data.size)
        codec.status()
        got = d_pts.cpu().numpy()
        assert np.array_equal(got[mis_out:mis_out + data.size], want[: data.size]), (number, "device resident", mis_in, mis_out)
        assert np.all(got[:mis_out] == FILL) and np.all(got[mis_out + data.size:] == FILL), (number, "device resident: outside")
    if every_leg or number % 11 == 0:
        # CLDN_HIP_FILL_ZERO: every covered byte is the oracle's, every uncovered one the buffer's old byte or 0
        c2 = native.Codec(plan)
        c2.set_decode_fill(True)
        got = c2.decode_lz4_host([body], [n], out=_filled(data.size))[0].reshape(n, step)
        ref = want[: n * step].reshape(n, step)
        covered = np.zeros(step, dtype=bool)
        for f in info.fields:
            covered[f.offset:f.offset + _SIZE[F(int(f.type))]] = True
        assert np.array_equal(got[:, covered], ref[:, covered]), (number, "fill zero: covered bytes")
        unc = got[:, ~covered]
        assert np.all((unc == FILL) | (unc == 0)), (number, "fill zero: uncovered bytes")
        c2.close()
    if every_leg or number % 4 == 0:
        # the library's OWN blocks, both parameter sets, device-resident from end to end
        d_in = torch.from_numpy(data.copy()).to(dev)
        for stage2 in (1, 2):
            codec.set_stage2(stage2)
            cap = plan.stage2_bound(n, stage2)
            d_stream = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
            d_off = torch.zeros(2, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
            codec.encode_device(d_in.data_ptr(), np.array([n], dtype=np.uint64), d_stream.data_ptr() + 5, cap, d_off.data_ptr())
            codec.status()
            offs = d_off.cpu().numpy().astype(np.uint64)
            codec.set_stage2(0)
            d_pts = torch.full((max(1, data.size),), FILL, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
            codec.decode_lz4_device(d_stream.data_ptr() + 5, offs, np.array([n], dtype=np.uint64), d_pts.data_ptr(), data.size)
            codec.status()
            assert np.array_equal(d_pts.cpu().numpy()[: data.size], want[: data.size]), (number, "own blocks", stage2)
    if every_leg or number % 6 == 0:
        # STALE SLOTS: a large cloud, then a cloud of the same schema with fewer and smaller chunks, then the large one again on
        # one codec, plain stage-1 calls in between (the launch hints of one route feed the other)
        n_small = max(1, n // 3)
        small = data[: n_small * step]
        s1_small = oracle.encode_stage1(info, small)
        want_small = oracle.decode_stage1(info, s1_small, n_small, fill=FILL)
        body_small = B.body_of(s1_small)
        c3 = native.Codec(plan)
        for _round in range(2):
            assert np.array_equal(c3.decode_lz4_host([body], [n], out=_filled(data.size))[0], want), (number, "stale slots: large")
            assert np.array_equal(c3.decode_host([s1_small], [n_small], out=_filled(small.size))[0], want_small), (number, "stale slots")
            assert np.array_equal(c3.decode_lz4_host([body_small], [n_small], out=_filled(small.size))[0], want_small), (number, "stale slots: small")
            assert np.array_equal(c3.decode_host([s1], [n], out=_filled(data.size))[0], want), (number, "stale slots")
        assert np.array_equal(c3.decode_lz4_host([body, body_small], [n, n_small], out=_filled(data.size + small.size))[1], want_small)
        c3.close()
    if every_leg or number % 7 == 0:
        # the point kernel's launch shape: chained, 2 and 16 workgroups per chunk
        for parts in (1, 2, 16):
            c4 = native.Codec(plan)
            assert c4.decode_split(parts) == 0
            got = c4.decode_lz4_host([body, body], [n, n], out=_filled(2 * data.size))
            assert np.array_equal(got[0], want) and np.array_equal(got[1], want), (number, "split", parts)
            c4.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _IDS, ids=_ID_NAMES)
def test_decode_lz4_equals_the_oracle(oracle, cid):
    from cloudini_amd import native
    info, data, number, n, s1, body = _case(oracle, cid)
    want = oracle.decode_stage1(info, s1, n, fill=FILL)
    plan = native.Plan(info)
    codec = native.Codec(plan)
    assert np.array_equal(codec.decode_host([s1], [n], out=_filled(data.size))[0], want), cid
    base_stats = codec.decode_stats()
    got = codec.decode_lz4_host([body], [n], out=_filled(data.size))[0]
    assert np.array_equal(got, want), (cid, [(f.name, int(f.type), f.offset, f.resolution) for f in info.fields], info.point_step,
                                       int(info.encoding_opt), info.version)
    stats = codec.decode_stats()
    assert n == 0 or sum(stats) > 0
    _no_new_serial_chunks(stats, base_stats)
    if n:
        # every leg for every second schema family; a fixed share of the legs for the other families, the very wide clouds (seconds
        # per leg) and the fuzz seeds
        pick = number // 4 + 2 if cid[0] == "wide" else number
        _legs(oracle, codec, plan, info, data, n, s1, body, want, pick, every_leg=cid[0] == "family" and number % 2 == 0)
    codec.close()


_MIRROR_IDS = [cid for k, cid in enumerate(_IDS) if k % 8 == 1]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _MIRROR_IDS, ids=[f"{a}-{b}" for a, b in _MIRROR_IDS])
def test_host_mirror_with_the_switch_on_equals_the_oracle(oracle, cid):
    from cloudini_amd import api
    info, data, _number, n, s1, body = _case(oracle, cid)
    linfo = B.lz4_info(info).copy(width=n, height=1)
    dec = api.PointcloudDecoder()
    assert not api.device_lz4_decode()
    off = dec.decode(linfo, body, fill=FILL)
    off_zero = dec.decode(linfo, body, output_is_zero=True)
    api.set_device_lz4_decode(True)
    try:
        on = dec.decode(linfo, body, fill=FILL)
        on_zero = dec.decode(linfo, body, output_is_zero=True)
    finally:
        api.set_device_lz4_decode(False)
    want = oracle.decode_stage1(info, s1, n, fill=FILL)[: data.size]
    assert np.array_equal(on, want) and np.array_equal(off, want), cid
    assert np.array_equal(on_zero, off_zero) and np.array_equal(on_zero, oracle.decode_stage1(info, s1, n, fill=0)[: data.size]), cid


def _expect(codec, native, oracle, info, bodies, counts, what):
    """The call's verdict and bytes are the model's; the error text names LZ4 exactly when a block is refused."""
    want = _model_batch(oracle, info, bodies, counts, FILL)
    step = info.point_step
    out = _filled(sum(counts) * step)
    if want is None:
        with pytest.raises(native.CloudiniHipError) as e:
            codec.decode_lz4_host(bodies, counts, out=out)
        assert e.value.code == -6, what
        cap = B.capacity_of(oracle, info)
        lz4_refusal = any(B.refused_block(b, n, cap) for b, n in zip(bodies, counts))
        assert ("LZ4 decompression failed" in str(e.value)) == lz4_refusal, (what, str(e.value))
        assert lz4_refusal or "stage-1" in str(e.value), (what, str(e.value))
        return False
    got = codec.decode_lz4_host(bodies, counts, out=out)
    for k, w in enumerate(want):
        assert np.array_equal(got[k], w), (what, "cloud", k)
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _DAMAGE_IDS, ids=[f"{a}-{b}" for a, b in _DAMAGE_IDS])
def test_damaged_lz4_bodies_decode_like_the_model(oracle, cid):
    from cloudini_amd import native
    info, data, number, n, s1, body = _case(oracle, cid)
    if body.size < 8:
        return
    want = oracle.decode_stage1(info, s1, n, fill=FILL)
    codec = native.Codec(native.Plan(info))
    for kind in B.DAMAGE_KINDS:
        bad = B.damage(kind, number, s1, body)
        if not _expect(codec, native, oracle, info, [bad], [n], (cid, kind)):
            # the codec decodes an intact body right after a reject
            assert np.array_equal(codec.decode_lz4_host([body], [n], out=_filled(data.size))[0], want), (cid, kind, "after the reject")
    codec.close()


@pytest.mark.gpu
def test_chain_table_decodes_like_the_model(oracle):
    from cloudini_amd import native
    info, table = chain_table(oracle)
    codec = native.Codec(native.Plan(info))
    accepted = 0
    for name, bodies, counts in table:
        ok = _expect(codec, native, oracle, info, bodies, counts, name)
        assert ok == (name in CHAIN_ROWS_ACCEPTED), name
        accepted += ok
        assert _expect(codec, native, oracle, info, table[1][1], table[1][2], "intact batch behind: " + name)
    assert accepted == len(CHAIN_ROWS_ACCEPTED)
    codec.close()


_MIRROR_DAMAGE_IDS = _DAMAGE_IDS[2::8]


@pytest.mark.gpu
def test_host_mirror_reports_damaged_bodies_like_the_model_and_the_reference(reflib, oracle):
    """With the switch on, PointcloudDecoder.decode raises exactly where the model rejects; with the switch off, exactly where
    the reference rejects. The two differ only where the strict block rules are stricter than liblz4."""
    from cloudini_amd import api
    dec = api.PointcloudDecoder()
    total = stricter = small = 0
    for cid in _MIRROR_DAMAGE_IDS:
        info, data, number, n, s1, body = _case(oracle, cid)
        if body.size < 8:
            continue
        linfo = B.lz4_info(info).copy(width=n, height=1)
        for kind in B.DAMAGE_KINDS:
            bad = B.damage(kind, number, s1, body)
            cap = B.capacity_of(oracle, info)
            want = B.model(oracle, info, bad, n, cap, FILL)
            ref = _ref_decode(reflib, info, bad, n, FILL)
            total += 1
            results = {}
            for on in (False, True):
                api.set_device_lz4_decode(on)
                try:
                    results[on] = dec.decode(linfo, bad, fill=FILL)
                except RuntimeError:
                    results[on] = None
                finally:
                    api.set_device_lz4_decode(False)
            assert (results[True] is None) == (want is None), (cid, kind, "switch on")
            blocks = B.walk(bad, n)
            if blocks is not None and any(len(R.lz4_decompress_safe(blk, cap) or b"") > n * info.point_step for blk in blocks):
                # a chunk larger than the cloud's points: the reference's own buffer is too small for it
                # (lz4_body.reference_buffer_too_small), the mirror's is not -- with liblz4 it decodes what the model decodes
                small += 1
                assert ref is None and (want is None or results[False] is not None), (cid, kind, "switch off")
            else:
                assert (results[False] is None) == (ref is None), (cid, kind, "switch off")
            if want is not None:
                assert np.array_equal(results[True], want[: data.size]) and np.array_equal(results[False], want[: data.size]), (cid, kind)
            elif results[False] is not None:
                stricter += 1
                assert B.refused_block(bad, n, cap), (cid, kind)   # (only the block rules may be stricter)
                assert ref is None or np.array_equal(results[False], ref), (cid, kind)
    print(f"{total} damaged bodies through the host mirror: {stricter} accepted with liblz4 and refused with the device decode; "
          f"{small} with a chunk larger than the reference's buffer")
    assert total >= 100
