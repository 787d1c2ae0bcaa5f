"""GPU: the DeltaVarint arm of the section decoders (decode_sections_core in k_decode_sections, k_decode_tail, k_decode_sections_cols:
the tile walker dv_stream with one 64-bit integer op) on the constructed grid of tests/dv_section_cases.py, one test per row so that a
failure names it. tests/test_dv_section_cases.py (CPU) proves that every row is what its name says.

Per row: the decoded bytes are the oracle's (a 0x3C pre-fill shows untouched bytes), decode_stats() says that the parallel kernels took
every chunk's regular stream AND sections -- byte parity alone cannot see a parallel path that gives up, the serial decoder produces
the same bytes -- and a second decode on the same codec, with the first call's hints in place, gives the same."""
import numpy as np
import pytest

import dv_section_cases as DC

pytestmark = pytest.mark.gpu

FILL = 0x3C
_prepared = {}


def _prep(oracle, row):
    """(stream, the oracle's decode) -- once per row"""
    if row.name not in _prepared:
        stream = row.stream(oracle)
        _prepared[row.name] = (stream, oracle.decode_stage1(row.info(), stream, row.n, fill=FILL) if row.error is None else None)
    return _prepared[row.name]


def _first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return int(d[0]) if d.size else -1


@pytest.mark.parametrize("row", DC.WELL_FORMED, ids=[r.name for r in DC.WELL_FORMED])
def test_decode(oracle, row):
    from cloudini_amd import native
    stream, want = _prep(oracle, row)
    codec = native.Codec(native.Plan(row.info()))
    for call in range(2):
        out = np.full(row.n * row.step, FILL, dtype=np.uint8)
        got = codec.decode_host([stream], [row.n], out=out)[0]
        assert np.array_equal(got, want), (call, "first difference at byte %d" % _first_diff(got, want))
        assert codec.decode_stats() == (len(row.ns), len(row.ns), 0, 0), (call, row.kernel)
    codec.close()


ALIGN_ROWS = [DC.BY_NAME[n] for n in ("a_lengths_cycle", "b_ten_bytes_3_in_front_of_the_first_edge", "c_section_bytes_5_mod_8", "g_tail_xyz_u64",
                                      "g_cols_dv_dv_XYZ_U16_U32")]


@pytest.mark.parametrize("row", ALIGN_ROWS, ids=[r.name for r in ALIGN_ROWS])
def test_decode_at_stream_residues(oracle, row):
    """The stream pointer handed to the decode call at residues 0..3 of a device address: the walker's dword loads give way to byte
    loads, the bytes and the counters stay."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    stream, want = _prep(oracle, row)
    codec = native.Codec(native.Plan(row.info()), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    size = row.n * row.step
    for res in range(4):
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
        assert codec.decode_stats() == (len(row.ns), len(row.ns), 0, 0), res
    codec.close()


@pytest.mark.parametrize("row", DC.MALFORMED, ids=[r.name for r in DC.MALFORMED])
def test_malformed(oracle, row):
    """The oracle refuses the chunk (ORC_ERR_TRUNCATED / ORC_ERR_CORRUPT, recorded in the row); the walker hands it back, the serial
    decoder raises CLDN_HIP_ERR_CORRUPT -- the one code the device has for both -- and the codec stays usable."""
    from cloudini_amd import native
    from oracle.binding import OracleError
    stream, _none = _prep(oracle, row)
    with pytest.raises(OracleError) as oe:
        oracle.decode_stage1(row.info(), stream, row.n)
    assert str(oe.value).endswith(": %d" % row.error)
    codec = native.Codec(native.Plan(row.info()))
    with pytest.raises(native.CloudiniHipError) as e:
        codec.decode_host([stream], [row.n], out=np.full(row.n * row.step, FILL, dtype=np.uint8))
    assert e.value.code == -6
    good = DC.BY_NAME["c_section_bytes_0_mod_8" if row.schema == "U64" else "d_section_at_residue_1"]
    g_stream, g_want = _prep(oracle, good)
    got = codec.decode_host([g_stream], [good.n], out=np.full(good.n * good.step, FILL, dtype=np.uint8))[0]
    assert np.array_equal(got, g_want)
    codec.close()


def test_int64_min_deltas(oracle):
    """The stream the oracle's encoder writes and its decoder refuses (deltas of +-2^63): the device agrees with the compiled
    reference, whose answer tests/test_dv_section_cases.py pins."""
    from cloudini_amd import native
    info, data, modes = DC.rejected_by_its_own_decoder()
    n = data.size // info.point_step
    stream = oracle.encode_stage1_continued(info, data, modes)
    codec = native.Codec(native.Plan(info))
    rejected = False
    try:
        codec.decode_host([stream], [n], out=np.full(data.size, FILL, dtype=np.uint8))
    except native.CloudiniHipError as e:
        assert e.code == -6
        rejected = True
    assert rejected == DC.REFERENCE_REJECTS_INT64_MIN_DELTAS
    codec.close()
