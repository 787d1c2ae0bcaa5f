"""The section grid on the CPU: tests/section_cases.py is what it says, tests/section_model.py writes the oracle's and the
reference's bytes. No GPU. tests/test_gpu_sections.py then holds the device against the model alone."""
import numpy as np
import pytest

import mode_model as M
from oracle import binding
import section_cases as SC
import section_model as S

F = SC.F
TYPES = SC.TYPES
IDS = [t.name for t in TYPES]


def _column(info, data):
    return M.column(info, data, M.adaptive_fields(info)[0])


@pytest.mark.parametrize("ftype", TYPES, ids=IDS)
def test_every_case_has_the_property_it_was_built_for(ftype):
    names = [c.name for c in SC.grid_of(ftype)]
    assert len(set(names)) == len(names)
    for c in SC.grid_of(ftype):
        v = SC.column_of(c, ftype)
        assert 1 <= v.size <= 2 * SC.CHUNK, c.name
        assert c.check(v), (ftype.name, c.name)
        for odd in (False, True):                                    # both layouts carry the same column
            info, data = SC.layout(c, ftype, odd)
            got, bpv = _column(info, data)
            assert np.array_equal(got, v) and bpv == SC.bits_of(ftype) // 8 and (info.point_step % 2 == 1) == odd, c.name


@pytest.mark.parametrize("ftype", TYPES, ids=IDS)
def test_model_sizes_equal_the_mode_model(ftype):
    bpv = SC.bits_of(ftype) // 8
    for c in SC.grid_of(ftype):
        v = SC.column_of(c, ftype)
        for s in range(0, v.size, SC.CHUNK):
            sec = v[s:s + SC.CHUNK]
            sizes = M.section_sizes(sec, bpv)
            got = [len(S.section_bytes(sec, bpv, ftype, m)) for m in S.MODES]
            assert got == sizes and max(got) < SC.SECTION_STRIDE, (ftype.name, c.name, s)


@pytest.mark.parametrize("ftype", TYPES, ids=IDS)
def test_model_streams_equal_the_oracle_under_every_mode(oracle, ftype):
    count = 0
    for c in SC.grid_of(ftype):
        for odd in (False, True):
            info, data = SC.layout(c, ftype, odd)
            n = data.size // info.point_step
            for m in S.MODES:
                got = S.stream_bytes(info, data, [m])
                assert got == oracle.encode_stage1_continued(info, data, [m]).tobytes(), (ftype.name, c.name, odd, m)
                if (c.name, m) in SC.UNDECODABLE:
                    with pytest.raises(binding.OracleError):
                        oracle.decode_stage1(info, np.frombuffer(got, np.uint8), n)
                    continue
                back = oracle.decode_stage1(info, np.frombuffer(got, np.uint8), n, fill=0xA5)   # (the padding of cases.pack)
                assert back.tobytes() == data.tobytes(), (ftype.name, c.name, odd, m)
            count += 4
    assert count == 8 * len(SC.grid_of(ftype)) >= 8 * 60


@pytest.mark.parametrize("ftype", TYPES, ids=IDS)
def test_model_streams_against_the_reference(reflib, ftype):
    """The reference's encoder writes the model's stream under the mode its own probe commits, and its decoder returns the
    input from the model's stream under every mode."""
    committed = set()
    for c in SC.grid_of(ftype):
        info, data = SC.layout(c, ftype, False)
        v, bpv = _column(info, data)
        probe = M.select(M.section_sizes(v[:M.PROBE], bpv))
        committed.add(probe)
        assert S.stream_bytes(info, data, [probe]) == reflib.encode_stage1(info, data).tobytes(), (ftype.name, c.name, probe)
        for m in S.MODES:
            stream = np.frombuffer(S.stream_bytes(info, data, [m]), np.uint8)
            if (c.name, m) in SC.UNDECODABLE:                          # the reference refuses what it wrote itself
                with pytest.raises(binding.OracleError, match="NaN marker"):
                    reflib.decode_noheader(info, stream)
                continue
            assert reflib.decode_noheader(info, stream).tobytes() == data.tobytes(), (ftype.name, c.name, m)
    assert committed == set(S.MODES), committed                       # the reference itself wrote every kind of section


def test_framing_of_regular_fields_in_front_of_the_sections(oracle):
    """stream_bytes with a regular stream: three quantised floats and a byte in front of two sections."""
    n = 40000
    i = np.arange(n)
    fields = [("x", 0, F.FLOAT32, 0.5), ("y", 4, F.FLOAT32, 0.5), ("z", 8, F.FLOAT32, 0.5), ("b", 12, F.UINT8, None),
              ("r", 13, F.UINT16, None), ("t", 15, F.INT64, None)]
    info = SC.cases.make_info(fields, 23, n)
    cols = {"x": (i % 50 * 0.5).astype(np.float32), "y": (-(i % 7) * 1.5).astype(np.float32), "z": np.zeros(n, np.float32),
            "b": (i % 251).astype(np.uint8), "r": (i // 9).astype(np.uint16), "t": (i * 1000003).astype(np.int64)}
    data = SC.cases.pack(info, cols, n)
    for modes in ([0, 0], [1, 2], [3, 1], [2, 3]):
        assert S.stream_bytes(info, data, modes) == oracle.encode_stage1_continued(info, data, modes).tobytes(), modes


# ---- the coverage table: asserted, not printed -------------------------------------------------------------------------

def _reaches(case, v, bpv, edge):
    """Whether the column reaches the edge, recomputed from the model (never from the case's own label)."""
    first = v[:SC.CHUNK]
    if edge == "thread":   # a run of two or more values or differences whose head lies on value 32k - 1, 32k or 32k + 1, k >= 1
        return any(((l >= 2) & (s >= 31) & np.isin(s % 32, (31, 0, 1))).any() for s, l in (SC._runs_at(first, False), SC._runs_at(first, True)))
    if edge == "tile":     # a 1024-value tile without a run head
        return any((np.add.reduceat(SC._heads(first, d).astype(int), np.arange(0, first.size, 1024)) == 0).any() for d in (False, True))
    if edge == "quarter":  # a DeltaVarint section of more than one quarter with tokens of more than one length
        return first.size > 8192 and np.unique(M._varint64_len(S.deltas(first))).size > 1
    if edge == "residue":  # a DeltaVarint section that ends at most one byte from a 16-byte edge
        return (1 + int(M._varint64_len(S.deltas(first)).sum())) % 16 in (0, 1, 15)
    if edge == "token":    # the longest varint of the width, or a 3-byte run length
        return int(M._varint64_len(S.deltas(first)).max()) == SC.max_delta_token_bytes(bpv) or first.size == SC.CHUNK and \
            (SC._runs_at(first, False)[1].max() >= 16384 or SC._runs_at(first, True)[1].max() >= 16384)
    if edge == "capacity":  # at least as many distinct values as the smallest table holds
        return np.unique(first).size >= SC.S2_PAL_CAPACITY
    raise KeyError(edge)


@pytest.mark.parametrize("ftype", TYPES, ids=IDS)
def test_coverage_table(ftype):
    bits = SC.bits_of(ftype)
    grid = SC.grid_of(ftype)
    cols = {c.name: SC.column_of(c, ftype) for c in grid}
    for c in grid:                                                   # a label is a claim: the model confirms each one
        for edge in c.edges:
            assert _reaches(c, cols[c.name], bits // 8, edge), (ftype.name, c.name, edge)
    for edge in SC.EDGES:                                            # every edge, at every width
        assert any(edge in c.edges for c in grid), (ftype.name, edge)
    uniques = [max(np.unique(cols[c.name][s:s + SC.CHUNK]).size for s in range(0, cols[c.name].size, SC.CHUNK)) for c in grid]
    # every (writer, mode) pair: a test of tests/test_gpu_sections.py that exists, and at least one case it sends there
    import test_gpu_sections as G
    for (writer, mode), routes in SC.ROUTES.items():
        mine = [(test, takes) for test, widths, takes in routes if bits in widths]
        assert mine or (writer in ("W1", "W5") and bits == 64) or (writer == "W4" and bits < 64), (ftype.name, writer, mode)
        for test, takes in mine:
            assert callable(getattr(G, test)), test
            assert any(takes(c.name, u) for c, u in zip(grid, uniques)), (ftype.name, writer, mode, test)
    assert G.WIDE_CASES is SC.WIDE_CASES and G.STALE_CASES is SC.STALE_CASES
    assert set(SC.WIDE_CASES) | set(SC.STALE_CASES) <= {c.name for c in grid}
    # both sides of every table capacity
    for cap in (SC.S2_PAL_CAPACITY, SC.PAL_CAPACITY):
        assert cap in uniques and cap + 1 in uniques, (ftype.name, cap)
    refused = [c.name for c in grid if c.outcome == SC.REFUSED]
    assert len(refused) == (1 if bits == 64 else 0), refused


def test_the_pal32_column_that_is_refused():
    v, check = SC.pal32_refused_column()
    info, data = SC.MC.layout(v, F.UINT32, False)
    assert check(_column(info, data)[0])
