"""CPU: the grid of tests/points_token_cases.py is what it says. For every row, at every address residue a0 the GPU test uses it at:
the predicate holds on the oracle's bytes, the oracle's decode gives the row's cloud back, the compiled reference writes the same
stream (where the row leaves the section modes to the encoder) and decodes it to the same bytes. The union of the rows covers the
position sets the grid is about, and the piece model agrees with a byte-by-byte walk. tests/test_gpu_points_tokens.py runs the rows
on the device."""
import numpy as np
import pytest

import points_token_cases as PC

FILL = 0x3C


def a0s_of(row):
    """every residue the GPU test builds the row for"""
    if row in PC.SUBSET:
        return tuple(range(16))
    return row.a0s


def _same_points(got, cloud, row, n):
    """the fields are the cloud's bit for bit (the deltas are exact multiples of the resolution), NaN for NaN; the rest keeps the fill"""
    covered = np.zeros(row.step, dtype=bool)
    for f in row.fields:
        covered[f[1]:f[1] + np.dtype(PC.cases._NP[f[2]]).itemsize] = True
    mask = np.tile(covered, n)
    g, c = got[mask].copy(), cloud[mask].copy()
    if not np.array_equal(g, c):
        # NaN payloads may differ: compare as floats per float field
        for f in row.fields[:row.nops]:
            a = np.ndarray(n, dtype="<f4", buffer=got.tobytes(), offset=f[1], strides=row.step)
            b = np.ndarray(n, dtype="<f4", buffer=cloud.tobytes(), offset=f[1], strides=row.step)
            if not np.array_equal(a, b, equal_nan=True):
                return False
        for f in row.fields[row.nops:]:
            dt = PC.cases._NP[f[2]]
            a = np.ndarray(n, dtype=dt, buffer=got.tobytes(), offset=f[1], strides=row.step)
            b = np.ndarray(n, dtype=dt, buffer=cloud.tobytes(), offset=f[1], strides=row.step)
            if not np.array_equal(a, b):
                return False
    return bool(np.all(got[~mask] == FILL))


@pytest.mark.parametrize("row", PC.ROWS, ids=[r.name for r in PC.ROWS])
def test_row_is_what_its_name_says(oracle, row):
    for a0 in a0s_of(row):
        streams, ns, clouds = row.streams(oracle, a0)
        M = row.models(streams, ns, a0)
        assert M[0].a0 == a0 and len(M) == sum(len(PC.chunk_points(n)) for n in ns)
        assert row.pred(M, a0), a0
        assert row.handback or PC.plain(M, a0)
        for m in M:       # what the kernel's geometry promises
            assert max(m.halo_tokens, default=0) <= row.nops - 1 and max(m.halo_bytes, default=0) <= 4 * (row.nops - 1) or row.handback
            assert max((k for _f, k in m.owned), default=0) <= (PC.PIECE + row.nops - 1) // row.nops
            assert m.cnt.max(initial=0) + 16 <= PC.SLOTS
        for stream, n, cloud in zip(streams, ns, clouds):
            got = oracle.decode_stage1(row.info(n), stream, n, fill=FILL)
            assert _same_points(got, cloud, row, n), a0
        if row.sections and row.modes is not None:
            for stream, m in zip(streams, M):      # the forced mode byte stands behind the regular stream
                assert m.payload[m.reg_end] == row.modes[0]


@pytest.mark.parametrize("row", PC.ROWS, ids=[r.name for r in PC.ROWS])
def test_reference_agrees(oracle, reflib, row):
    """The compiled reference writes the same stream (rows with forced section modes: it would choose its own) and decodes the
    oracle's bytes to the same points."""
    for a0 in a0s_of(row):
        streams, ns, clouds = row.streams(oracle, a0)
        for stream, n, cloud in zip(streams, ns, clouds):
            info = row.info(n)
            if row.modes is None:
                assert np.array_equal(reflib.encode_stage1(info, cloud), stream), a0
            assert np.array_equal(reflib.decode_noheader(info, stream, fill=FILL), oracle.decode_stage1(info, stream, n, fill=FILL)), a0


TWINNED = [r for r in PC.ROWS if not r.sections]


@pytest.mark.parametrize("row", TWINNED, ids=[r.name for r in TWINNED])
def test_the_pinned_twin_carries_the_rows_tokens(oracle, reflib, row):
    """PC.pinned(row): the same token stream in front of a forced Palette section, at every a0 the GPU test uses -- the regular stream
    of every chunk is the row's payload byte for byte, the mode byte behind it is 1, the oracle and the compiled reference decode it
    to the twin's cloud."""
    twin = PC.pinned(row)
    assert twin.base is row and twin.schema == PC.PINNED[row.nops] and twin.modes == [1]
    for a0 in a0s_of(row):
        streams, ns, clouds = twin.streams(oracle, a0)
        M = twin.models(streams, ns, a0)
        b_streams, b_ns, _c = row.streams(oracle, a0)
        assert M[0].a0 == a0 and ns == b_ns
        assert twin.pred(M, a0) and PC.carries_the_base_tokens(M, row.models(b_streams, b_ns, a0)), a0
        for stream, n, cloud in zip(streams, ns, clouds):
            got = oracle.decode_stage1(twin.info(n), stream, n, fill=FILL)
            assert _same_points(got, cloud, twin, n), a0
            assert np.array_equal(reflib.decode_noheader(twin.info(n), stream, fill=FILL), got), a0


def _union(oracle, rows, what):
    got = set()
    for row in rows:
        a0 = row.a0s[0]
        streams, ns, _c = row.streams(oracle, a0)
        for m in row.models(streams, ns, a0):
            got |= getattr(m, what)()
    return got


def test_the_grid_covers_the_unit_positions(oracle):
    """every (position in the unit, token length) pair in lane 1's unit, in a unit between and in lane 62's unit: 64 pairs x 3 places"""
    for nops in (3, 4):
        got = _union(oracle, [r for r in PC.ROWS if r.family == "unit" and r.nops == nops], "unit_positions")
        want = {(place, pos, L) for place in (1, 0, PC.UNITS) for pos in range(16) for L in range(1, 5)}
        assert want <= got, sorted(want - got)
        assert sum(1 for (_p, pos, L) in want if pos < L - 1) == 3 * 6     # the tokens that straddle two units


def test_the_grid_covers_the_piece_boundaries(oracle):
    """every (length, bytes in front of a piece boundary, index in the point): s = 0..L, so a token that ends on a piece's last byte is in"""
    for nops in (3, 4):
        got = _union(oracle, [r for r in PC.ROWS if r.family == "boundary" and r.nops == nops], "boundary_splits")
        want = {(L, s, o) for L in range(1, 5) for s in range(L + 1) for o in range(nops)}
        assert want <= got, sorted(want - got)
    got = _union(oracle, [r for r in PC.HANDBACK], "boundary_splits")
    assert {s for (L, s, _o) in got if L == 5} >= set(range(5))


def test_the_table_has_every_family():
    names = set(PC.BY_NAME)
    assert {r.family for r in PC.ROWS} == set(PC.FAMILIES)
    for nops in (3, 4):
        assert {"halo_%d_tokens_nops%d" % (k, nops) for k in range(nops)} <= names
        assert {"first_token_len%d_a0_%d_nops%d" % (L, a, nops) for L in range(1, 5) for a in range(16)} <= names
        assert {"tiny_%d_points_a0_%d_nops%d" % (n, a, nops) for n in (1, 2, 5) for a in range(16)} <= names
        assert {"last_piece_%d_bytes_nops%d" % (k, nops) for k in (1, 15, 16, 17, 991, 992)} <= names
        assert len([r for r in PC.ROWS if r.family == "nan" and r.nops == nops]) == 8
    assert {"regular_end_at_%s_%s" % (k, s) for k in ("990", "991", "0", "1", "last_byte_of_the_halo_unit") for s in ("XYZ_U16", "XYZ_U32")} <= names
    assert {r.family for r in PC.SUBSET} == set(PC.FAMILIES) - {"first_token", "tiny", "handback"}
    assert {(r.family, r.nops) for r in PC.SUBSET} >= {(f, k) for f in ("unit", "boundary", "halo", "last", "nan", "density", "carry") for k in (3, 4)}
    assert len(PC.HANDBACK) == 14 and all(r.schema in ("XYZ", "XYZW") and r.reports == ((1, 0, 0, 0), "payload size", None) and
                                        PC.pinned(r).reports == ((1, 1, 0, 0), "regular end", 1) for r in PC.HANDBACK)
    # only the ring rows need a full chunk
    assert all(r.family == "ring" or len(c) <= 12000 * r.nops for r in PC.ROWS for c, _s in r.build(r.a0s[0]))


def test_lengths_follow_from_the_deltas():
    for L in range(1, 6):
        mag = 0 if L == 1 else 1 << (7 * (L - 1) - 1)
        for d in (mag, -mag):
            zz = ((d << 1) ^ (d >> 63)) & ((1 << 64) - 1)
            assert PC.varint_len(zz + 1) == L
    x = PC.lanes_for([2, 0, 3, 4, 1, 5, 0, 2, 2], 3)
    assert np.isnan(x[0, 1]) and np.isnan(x[2, 0]) and x[0, 0] == 32.0 and x[2, 1] == 32.0 and x[1, 2] == float((1 << 26) + (1 << 12))


WALK_SIZES = (1, 2, 15, 16, 17, 991, 992, 993, 1007, 1008, 1009, 2500, 5000)


@pytest.mark.parametrize("nops", (3, 4))
@pytest.mark.parametrize("size", WALK_SIZES)
def test_the_piece_model_equals_a_serial_walk(size, nops):
    """random bytes (tokens of any length) at several a0, with and without bytes behind the regular stream; sizes around a unit, a
    piece and a piece with its halo"""
    for k, a0 in enumerate((0, 1, 7, 15)):
        rs = np.random.RandomState(1000 * size + 10 * nops + k)
        payload = rs.randint(0, 256, size).astype(np.uint8)
        payload[rs.rand(size) < 0.45] &= 0x7F
        payload[-nops:] &= 0x7F                                   # at least one point, whatever the size (size 1, 2: padded below)
        if size < nops:
            payload = np.concatenate([payload, np.full(nops - size, 0x01, dtype=np.uint8)])
        n_ends = int(np.sum(payload < 0x80))
        n = n_ends // nops if k % 2 else max(1, n_ends // nops // 2)    # (even k: bytes that are no tokens of the regular stream follow)
        assert n >= 1
        m = PC.Model(payload, a0, nops, n)
        ends, reg_end, T0, cnt, owner, row, halo, halo_bytes = PC.serial_model(payload, a0, nops, n)
        assert m.ends.tolist() == ends and m.reg_end == reg_end
        assert m.T0.tolist() == T0 and m.cnt.tolist() == cnt
        assert m.owner.tolist() == owner and m.row.tolist() == row
        owns = [k_ > 0 for _f, k_ in m.owned]
        assert [h for h, o in zip(m.halo_tokens, owns) if o] == [h for h, o in zip(halo, owns) if o]
        assert [h for h, o in zip(m.halo_bytes, owns) if o] == [h for h, o in zip(halo_bytes, owns) if o]
        assert sum(k_ for _f, k_ in m.owned) == n
