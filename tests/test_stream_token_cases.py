"""CPU: the grid of tests/stream_token_cases.py is what it says. For every row, at every address residue a0 the GPU test uses it at:
the predicate holds on the oracle's bytes and the oracle's decode gives the row's cloud back. Every pinned twin carries its base row's
regular stream byte for byte, the piece model agrees with a byte-by-byte walk, every schema takes the route its rows are about --
through decode_route() itself -- and the union of the rows reaches every value the grid is about (counted; a value no row reaches
fails). tests/test_gpu_stream_tokens.py runs the rows on the device."""
import numpy as np
import pytest

import stream_token_cases as SC

FILL = 0x3C
_built = {}


def built(oracle, row, a0):
    """(streams, ns, clouds, models) -- once per (row, schema, a0)"""
    key = (row.name, row.schema.name, a0)
    if key not in _built:
        streams, ns, clouds = row.streams(oracle, a0)
        _built[key] = (streams, ns, clouds, row.models(streams, ns, a0))
    return _built[key]


def _same_points(got, cloud, S, n):
    """the fields are the cloud's bit for bit (the deltas are exact multiples of the resolution; a NaN is the decoder's quiet NaN, which
    is numpy's); the rest keeps the fill"""
    covered = np.zeros(S.step, dtype=bool)
    for f in S.fields:
        covered[f[1]:f[1] + SC._SIZE[f[2]]] = True
    mask = np.tile(covered, n)
    return np.array_equal(got[mask], cloud[mask]) and bool(np.all(got[~mask] == FILL))


@pytest.mark.parametrize("row", SC.ROWS, ids=[r.name for r in SC.ROWS])
def test_row_is_what_its_name_says(oracle, row):
    S = row.schema
    for a0 in row.a0s:
        streams, ns, clouds, M = built(oracle, row, a0)
        assert M[0].a0 == a0 and len(M) == sum(len(SC.chunk_points(n)) for n in ns)
        assert row.pred(M, a0), a0
        for m in M:       # what the kernel's geometry promises
            assert m.point_len.max(initial=0) <= SC.MAX_POINT and m.lens.max(initial=0) <= 10
            assert int(m.owned.max(initial=0)) <= SC.PIECE + 1 and int(m.T0.max(initial=0)) < (1 << 19)
            assert m.reg_end == len(m.payload) or row.sections
            assert not row.sections or m.reg_end < len(m.payload)
        for stream, n, cloud in zip(streams, ns, clouds):
            assert _same_points(oracle.decode_stage1(row.info(n), stream, n, fill=FILL), cloud, S, n), a0


TWINNED = [r for r in SC.ROWS if r.schema.name in SC.TWIN]


@pytest.mark.parametrize("row", TWINNED, ids=[r.name for r in TWINNED])
def test_the_pinned_twin_carries_the_rows_tokens(oracle, row):
    twin = SC.pinned(row)
    assert twin.base is row and twin.schema.name == SC.TWIN[row.schema.name] and twin.schema.nops == row.schema.nops
    assert [o[:2] for o in twin.schema.ops] == [o[:2] for o in row.schema.ops] and len(twin.schema.adaptive) == 1
    for a0 in row.a0s:
        streams, ns, clouds, M = built(oracle, twin, a0)
        _s, b_ns, _c, base_M = built(oracle, row, a0)
        assert M[0].a0 == a0 and ns == b_ns
        assert SC.carries_the_base_tokens(M, base_M), a0
        assert all(m.reg_end < len(m.payload) for m in M)
        for stream, n, cloud in zip(streams, ns, clouds):
            assert _same_points(oracle.decode_stage1(twin.info(n), stream, n, fill=FILL), cloud, twin.schema, n), a0


@pytest.fixture(scope="module")
def route_shim(tmp_path_factory):
    import test_decode_route as TR
    return TR, TR.build_shim(tmp_path_factory.mktemp("stream_route"))


@pytest.mark.parametrize("name", sorted(SC.SCHEMAS))
def test_every_schema_takes_its_route(route_shim, name):
    TR, lib = route_shim
    S = SC.SCHEMAS[name]
    for n_chunks in (1, 2):
        _kernels, got = SC.check_route(TR, lib, S, n_chunks)
        if S.marker != "none":
            assert 0 < got["automaton_states"] <= (8 if S.marker == "automaton32" else 16)
        if S.route == "fixed":
            assert got["fixed_bytes"] == S.raw_bytes
    if S.route == "form":
        assert S.max_regular <= SC.MAX_POINT and got["automaton_states"] == 0


@pytest.mark.parametrize("name", sorted(SC.ROUTE_ONLY))
def test_plans_the_stream_kernel_does_not_get(route_shim, name):
    """nine ops, varints or raw fields: the serial decoder (the stream kernel's fixed_F path outside section mode has no plan)"""
    TR, lib = route_shim
    fields, version, enc, want = SC.ROUTE_ONLY[name]
    step = max(f[1] + SC._SIZE[f[2]] for f in fields)
    kernels, got = SC.selected_route(TR, lib, fields, step, version, enc)
    assert got["regular"] == want and "k_decode_stream_w" not in kernels and "k_decode_fixed" not in kernels


def test_the_schemas_cover_what_the_issue_lists():
    S = SC.SCHEMAS
    assert sorted(S[n].nops for n in SC.STREAM) == [1, 2, 3, 4, 5, 5, 6, 7, 8]
    assert [S[n].nops for n in SC.STREAM_V4] == [1, 8, 5] and all(S[n].version == 4 for n in SC.STREAM_V4)
    assert {S[n].marker for n in SC.BITMAP} == {"automaton32", "automaton64"}
    assert {s for n in SC.BITMAP + SC.FORM for t, s in S[n].form if t == "r"} == {1, 4, 8}
    assert sorted(min(S[n].max_regular, SC.MAX_POINT) > 64 for n in SC.FORM) == [False, False, False, True]
    # seven varints of 10 bytes and a raw field of 8: eight ops with a raw field have no more, and that form has 15 states (bitmap mode);
    # more than 16 states: six varints and two raw fields of 8
    assert max(S[n].max_regular for n in SC.BITMAP) == 78 and max(S[n].max_regular for n in SC.FORM) == 76
    assert S["QUAD"].raw_bytes == 16 and S["FIXED_8"].nops == 8 and S["FIXED_MIXED"].raw_bytes % 2 == 0 and S["FIXED_MIXED"].fields[0][1] == 1
    assert {len(S[n].adaptive) for n in SC.SECTION} == {1, 2}
    assert all(S[SC.TWIN[n]].route == "stream_cols" for n in SC.STREAM)


def test_the_table_is_complete(oracle):
    """counted over the models of every row at every a0 it runs at"""
    k0s, lens, a0s, keeps, shapes, markers, entries, sect_lens = set(), {}, set(), set(), set(), set(), set(), {}
    families = set()
    for row in SC.ROWS:
        S = row.schema
        families.add(row.family)
        for a0 in row.a0s:
            _st, _ns, _cl, M = built(oracle, row, a0)
            for m in M:
                a0s.add((S.route, m.a0))
                if S.route in ("stream", "stream_cols"):
                    k0s |= m.k0s
                cl = m.code_lens()
                for o in S.var_ops:
                    kind = (S.ops[o][0], S.ops[o][1])
                    lens.setdefault(kind, set()).update(np.unique(cl[:, o]).tolist())
                if S.sections == "side_by_side":
                    for sm, (bpv, _o, _i) in zip(SC.section_models(m), S.adaptive):
                        a0s.add(("section", sm.a0))
                        sect_lens.setdefault(bpv, set()).update(np.unique(sm.lens).tolist())
                if S.route == "form":
                    entries |= {e for e in m.entry[1:] if e is not None}
                    keeps |= set(m.keep[m.owned_form > 0].tolist())
                    shapes.add(min(S.max_regular, SC.MAX_POINT) <= 64)
                if S.marker != "none":
                    markers.add(S.marker)
    assert families == set(SC.FAMILIES)
    assert k0s == {(n, k) for n in range(1, 9) for k in range(n)}, sorted({(n, k) for n in range(1, 9) for k in range(n)} - k0s)
    want = {(SC.QF32, 4): 5, (SC.LF32, 4): 10, (SC.LF64, 8): 10, (SC.INT, 4): 5, (SC.INT, 8): 10}
    assert set(lens) == set(want)
    for kind, top in want.items():
        assert lens[kind] >= set(range(1, top + 1)), (kind, sorted(lens[kind]))
    # MODE 1: pieces entered at 0, 63, 64 and maxpt - 1 = 75; entries of 64 and more are read from the second candidate set
    assert entries >= {0, 63, 64, 75} and max(entries) < SC.MAX_POINT
    assert sect_lens[2] >= {1, 2, 3} and sect_lens[4] >= {1, 2, 3, 4, 5}
    for route in ("stream", "stream_bitmap", "form", "section"):
        assert {a for r, a in a0s if r == route} == set(range(16)), route
    assert keeps == {True, False} and shapes == {True, False}
    # all the marker kernels a plan of the C ABI can put in front of the stream kernel (k_mark_token_ends: none can, see the cases' docstring)
    assert markers == {"automaton32", "automaton64"}
    assert SC.HANDBACK == []


def _keep_stop_and_target(m, S, begin, last_v):
    """keep, stop and target_unit of the model from the serial walk's plain counts. keep: the values of the points that begin in the
    piece (4 bytes for a FloatN lane or an integer of at most 4 bytes, 8 otherwise, for an even number of points), rounded up to 8
    bytes, and one 64-bit marker mask per row of 64 points and op fit the 3456 bytes where the jump table was. Nothing on the device
    shows `keep`: both outcomes store the same bytes, the rows only make both happen."""
    value_bytes = sum(4 if (k == SC.QF32 or (k == SC.INT and sz <= 4)) else 8 for k, sz, _o, _i in S.ops)
    for p, k in enumerate(begin):
        values = (k + k % 2) * value_bytes
        values += -values % 8
        masks = -(-k // 64) * S.nops * 8
        assert bool(m.keep[p]) == (k > 0 and values + masks <= 3456), (p, k)
        assert bool(m.stop[p]) == (p > 0 and last_v is not None and last_v < p * SC.PIECE), p
    assert m.target_unit == (None if last_v is None else last_v % SC.PIECE // 16)
    assert m.owned_form.tolist() == begin


WALK_SIZES = (1, 2, 15, 16, 17, 1007, 1023, 1024, 1025, 1040, 2500, 5000)


@pytest.mark.parametrize("name", ("F1", "F2", "XYZ_D", "F8", "XYZ_R4_B", "I64x6_2X8"))
@pytest.mark.parametrize("size", WALK_SIZES)
def test_the_piece_model_equals_a_serial_walk(size, name):
    """random bytes at several a0, with and without bytes behind the regular stream"""
    S = SC.SCHEMAS[name]
    for k, a0 in enumerate((0, 1, 7, 15)):
        rs = np.random.RandomState(1000 * size + 10 * S.nops + k)
        payload = rs.randint(0, 256, size + 12 * S.max_regular).astype(np.uint8)
        payload[rs.rand(len(payload)) < 0.45] &= 0x7F
        payload[-12 * S.max_regular:] &= 0x7F                     # (enough ends for a few points, whatever the size)
        probe = SC.Model(payload, a0, SC.SCHEMAS["F1"], 1)
        if S.raw_bytes:
            n = max(1, size // S.max_regular)
        else:
            n_ends = int(np.sum(payload < 0x80))
            n = n_ends // S.nops if k % 2 else max(1, n_ends // S.nops // 2)
        assert probe.n_pieces >= 1 and n >= 1
        m = SC.Model(payload, a0, S, n)
        ends, reg_end, T0, cnt, owner, row, lane, k0, entry, owner_form, begin, last_v = SC.serial_model(payload, a0, S, n)
        _keep_stop_and_target(m, S, begin, last_v)
        assert m.ends.tolist() == ends and m.reg_end == reg_end
        assert m.T0.tolist() == T0 and m.cnt.tolist() == cnt
        assert m.owner.tolist() == owner and m.row.tolist() == row and m.lane.tolist() == lane
        assert m.k0_of_unit == k0
        assert m.owner_form.tolist() == owner_form and m.entry == entry
        assert int(m.owned.sum()) == n and int(m.owned_form.sum()) == n


def test_the_models_of_the_rows_equal_a_serial_walk(oracle):
    """the same on real streams: one row of every family and route"""
    seen = set()
    for row in SC.ROWS:
        key = (row.family, row.schema.route)
        a0 = row.a0s[0]
        if key in seen:
            continue
        _st, _ns, _cl, M = built(oracle, row, a0)
        m = M[0]
        if len(m.payload) > 20000:
            continue
        seen.add(key)
        ends, reg_end, T0, cnt, owner, rw, lane, k0, entry, owner_form, begin, last_v = SC.serial_model(m.payload, m.a0, row.schema, m.n)
        _keep_stop_and_target(m, row.schema, begin, last_v)
        assert m.ends.tolist() == ends and m.reg_end == reg_end and m.T0.tolist() == T0 and m.cnt.tolist() == cnt, row.name
        assert m.owner.tolist() == owner and m.row.tolist() == rw and m.lane.tolist() == lane and m.k0_of_unit == k0, row.name
        assert m.owner_form.tolist() == owner_form and m.entry == entry, row.name
    assert {f for f, _r in seen} == set(SC.FAMILIES)


def test_lengths_follow_from_the_deltas():
    for wide in (False, True):
        for L in range(1, 11 if wide else 6):
            mag = SC.magnitude(L, wide)
            for d in (mag, -mag):
                zz = ((d << 1) ^ (d >> 63)) & ((1 << 64) - 1)
                assert SC.varint_len(zz + 1) == L
    q, nan = SC.lane_ticks([2, 0, 3, 7, 1, 7, 2], False)
    assert nan.tolist() == [False, True] + [False] * 5 and q.tolist() == [64, 0, 8192, 3 << 40, 3 << 40, 0, -64]
    q, _nan = SC.lane_ticks([10, 10, 10, 10], True, signs=[1, 1, 1, 1])
    assert q.tolist() == [1 << 62, -(1 << 63), -(1 << 62), 0]
