"""GPU: the three hand-written Gorilla kernels -- k_gorilla_tokens (in front of the generic encoder), k_gorilla_windows + the Gorilla
TAIL of k_encode_fused (the piece kernel), k_decode_stream_w<12, 2> (the decoder) -- on the constructed grid of
tests/gorilla_cases.py, one test per row so that a failure names it. tests/test_gorilla_model.py (CPU) proves that every row is what
its name says and that the model's codec is the oracle's.

Encode: the stream's bytes are the oracle's, through every pipeline the schema has, alone and as the second cloud of a batch.
Decode: the bytes are the oracle's (untouched bytes included), twice on one codec, and the number of chunks the parallel decoder
handed to the serial one is EXACTLY the model's (gorilla_model.serial_expected): byte parity alone cannot see a parallel path that
gives up, the serial decoder produces the same bytes."""
import numpy as np
import pytest

import gorilla_cases as GC

pytestmark = pytest.mark.gpu

FILL = 0x5A
ENCODE_RUNS = [(r, p) for r in GC.EXPRESSIBLE for p in r.pipelines]
_prepared = {}


def _prep(oracle, row):
    """(stream, the oracle's decode, serial chunks by the model with the stream at a 16-byte aligned address) -- once per row"""
    if row.name not in _prepared:
        stream = row.stream(oracle)
        want = oracle.decode_stage1(row.info(), stream, row.n, fill=FILL)
        _prepared[row.name] = (stream, want, sum(c[1] for c in GC.layout(row, stream)))
    return _prepared[row.name]


def _companion(row):
    """A cloud of the same schema and another length, to stand in front of the row's in a batch."""
    for name in ("c_reuse_edges_", "j_2_in_a_batch_", "a_every_length_", "j_openers_62_65_", "j_openers_511_513_"):
        other = GC.BY_NAME.get(name + row.schema)
        if other is not None and other.n != row.n:
            return other
    raise KeyError(row.schema)


@pytest.mark.parametrize("row,pipeline", ENCODE_RUNS, ids=["%s-pipeline%d" % (r.name, p) for r, p in ENCODE_RUNS])
def test_encode(oracle, row, pipeline):
    from cloudini_amd import native
    stream, _want, _serial = _prep(oracle, row)
    cloud = row.cloud()
    other = _companion(row)
    other_stream = _prep(oracle, other)[0]
    codec = native.Codec(native.Plan(row.info()))
    assert codec.pipeline(pipeline) == pipeline or pipeline == 0      # (0: the route's own choice -- the WIDE rows)
    got = codec.encode_host([cloud])[0][0]
    assert got.size == stream.size and np.array_equal(got, stream), "first difference at byte %d" % _first_diff(got, stream)
    got = codec.encode_host([other.cloud(), cloud])[0]
    assert np.array_equal(got[0], other_stream), "the cloud in front: first difference at byte %d" % _first_diff(got[0], other_stream)
    assert np.array_equal(got[1], stream), "second of a batch: first difference at byte %d" % _first_diff(got[1], stream)
    codec.close()


def _first_diff(a, b):
    k = min(a.size, b.size)
    d = np.nonzero(a[:k] != b[:k])[0]
    return int(d[0]) if d.size else k


@pytest.mark.parametrize("row", GC.DECODE, ids=[r.name for r in GC.DECODE])
def test_decode(oracle, row):
    from cloudini_amd import native
    stream, want, serial = _prep(oracle, row)
    assert serial == row.serial
    codec = native.Codec(native.Plan(row.info()))
    for call in range(2):
        out = np.full(row.n * row.step, FILL, dtype=np.uint8)
        got = codec.decode_host([stream], [row.n], out=out)[0]      # (the stream lies at a 16-byte aligned device address)
        assert np.array_equal(got, want), (call, "first difference at byte %d" % _first_diff(got, want))
        stats = codec.decode_stats()
        assert stats[2] == serial and stats[0] == len(row.ns) - serial, (call, stats, serial)
    codec.close()


E_ROWS = [r for r in GC.WELL_FORMED if r.family in ("e", "d")] + [GC.BY_NAME["f_ten_bytes_3_in_front"], GC.BY_NAME["h_40_changes_in_the_second_piece"],
                                                                   GC.BY_NAME["h_39_changes_in_the_second_piece"]]


@pytest.mark.parametrize("row", E_ROWS, ids=[r.name for r in E_ROWS])
def test_decode_at_every_residue(oracle, row):
    """The stream at each of the 16 residues of a device address: a0 (the payload's address mod 16) takes every value -- the raw first
    value is recognised by `lane * 16 + i == a0`, and the pieces (so the model's count) move with it."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    stream, want, _serial = _prep(oracle, row)
    codec = native.Codec(native.Plan(row.info()), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    size = row.n * row.step
    for res in range(16):
        serial = sum(c[1] for c in GC.layout(row, stream, residue=res))
        buf = np.full(res + stream.size + 64, 0xEE, dtype=np.uint8)
        buf[res:res + stream.size] = stream
        d_stream = torch.from_numpy(buf).to(dev)
        assert d_stream.data_ptr() % 16 == 0
        d_out = torch.full((size,), FILL, dtype=torch.uint8, device=dev)
        codec.decode_device(d_stream.data_ptr() + res, np.array([0, stream.size], dtype=np.uint64), np.array([row.n], dtype=np.uint64),
                            d_out.data_ptr(), size, 0)
        codec.status()
        got = d_out.cpu().numpy()
        assert np.array_equal(got, want), (res, "first difference at byte %d" % _first_diff(got, want))
        stats = codec.decode_stats()
        assert stats[2] == serial and stats[0] == len(row.ns) - serial, (res, stats, serial)
    codec.close()


@pytest.mark.parametrize("row", GC.MALFORMED, ids=[r.name for r in GC.MALFORMED])
def test_malformed(oracle, row):
    """The oracle refuses the chunk; so does the device call (the piece gives up, the serial decoder raises), and the codec stays
    usable."""
    from cloudini_amd import native
    from oracle.binding import OracleError
    stream = row.stream(oracle)
    with pytest.raises(OracleError):
        oracle.decode_stage1(row.info(), stream, row.n)
    codec = native.Codec(native.Plan(row.info()))
    with pytest.raises(native.CloudiniHipError) as e:
        codec.decode_host([stream], [row.n], out=np.full(row.n * row.step, FILL, dtype=np.uint8))
    assert e.value.code == -6
    good = GC.BY_NAME["c_reuse_edges_A"]
    g_stream, g_want, _s = _prep(oracle, good)
    got = codec.decode_host([g_stream], [good.n], out=np.full(good.n * good.step, FILL, dtype=np.uint8))[0]
    assert np.array_equal(got, g_want)
    codec.close()
