"""CPU: the grid of tests/dv_section_cases.py is what it says. Every well-formed row round-trips through the oracle, its predicate holds
on the oracle's bytes, its sections carry the forced mode bytes; the compiled reference decodes the same bytes to the same points and
refuses the malformed rows the oracle refuses. tests/test_gpu_dv_sections.py runs the rows on the device."""
import numpy as np
import pytest

import dv_section_cases as DC
from oracle.binding import OracleError

FILL = 0x3C


@pytest.mark.parametrize("row", DC.WELL_FORMED, ids=[r.name for r in DC.WELL_FORMED])
def test_row_is_what_its_name_says(oracle, row):
    stream = row.stream(oracle)
    P = row.parse(stream)
    assert len(P) == len(row.ns)
    assert all([s.mode for s in c.sections] == row.modes for c in P)
    assert row.pred(P)
    cloud = row.cloud()
    got = oracle.decode_stage1(row.info(), stream, row.n, fill=FILL)
    # (bytes no field covers keep the fill; the fields are the cloud's)
    covered = np.zeros(row.step, dtype=bool)
    for f in row.fields:
        covered[f[1]:f[1] + np.dtype(DC.cases._NP[f[2]]).itemsize] = True
    mask = np.tile(covered, row.n)
    assert np.array_equal(got[mask], cloud[mask]) and np.all(got[~mask] == FILL)


def test_the_grid_covers_the_issue():
    names = set(DC.BY_NAME)
    assert {"a_len%d_%s" % (L, s) for L in range(1, 11) for s in ("U64", "I64")} <= names
    assert {"c_section_bytes_%d_mod_8" % r for r in range(8)} <= names and {"d_section_at_residue_%d" % r for r in range(8)} <= names
    assert {r.kernel for r in DC.WELL_FORMED} == {"k_decode_sections", "k_decode_tail", "k_decode_sections_cols"}
    assert len(DC.ROWS) <= 120 and max(r.n for r in DC.ROWS) <= DC.CHUNK + 1


def test_lengths_follow_from_the_deltas():
    for L in range(1, 11):
        d = [int(x) for x in DC.deltas_for([L, L])]
        for v in d:
            s = v - (1 << 64) if v >> 63 else v
            zz = ((s << 1) ^ (s >> 63)) & DC.M64
            assert DC.varint_len(zz + 1) == L, (L, v)


@pytest.mark.parametrize("row", DC.MALFORMED, ids=[r.name for r in DC.MALFORMED])
def test_malformed_rows_raise_the_recorded_error(oracle, row):
    stream = row.stream(oracle)
    with pytest.raises(OracleError) as e:
        oracle.decode_stage1(row.info(), stream, row.n)
    assert str(e.value).endswith(": %d" % row.error), e.value


@pytest.mark.parametrize("row", DC.ROWS, ids=[r.name for r in DC.ROWS])
def test_reference_agrees(oracle, reflib, row):
    """The compiled reference on the oracle's bytes (its own encoder would choose other modes): the same points, or a refusal."""
    stream = row.stream(oracle)
    if row.error is not None:
        with pytest.raises(OracleError):
            reflib.decode_noheader(row.info(), stream, fill=FILL)
        return
    assert np.array_equal(reflib.decode_noheader(row.info(), stream, fill=FILL), oracle.decode_stage1(row.info(), stream, row.n, fill=FILL))


def test_int64_min_deltas_encode_but_do_not_decode(oracle):
    info, data, modes = DC.rejected_by_its_own_decoder()
    stream = oracle.encode_stage1_continued(info, data, modes)
    assert stream[4] == 0
    with pytest.raises(OracleError) as e:
        oracle.decode_stage1(info, stream, data.size // 8)
    assert str(e.value).endswith(": -5")


def test_int64_min_deltas_by_the_reference(oracle, reflib):
    """What the compiled reference does with that stream is recorded in DC.REFERENCE_REJECTS_INT64_MIN_DELTAS; the GPU test holds the
    device to it."""
    info, data, modes = DC.rejected_by_its_own_decoder()
    stream = oracle.encode_stage1_continued(info, data, modes)
    try:
        reflib.decode_noheader(info, stream, fill=FILL)
        rejected = False
    except OracleError:
        rejected = True
    assert rejected == DC.REFERENCE_REJECTS_INT64_MIN_DELTAS
