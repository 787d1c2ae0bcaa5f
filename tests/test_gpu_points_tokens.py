"""GPU: k_decode_points_w (stage1_decode_wave.h), both launch shapes, on the constructed grid of tests/points_token_cases.py, one test
per row so that a failure names it. tests/test_points_token_cases.py (CPU) proves that every row, and every row's pinned twin, is what
it says at every address residue used here.

Per row: the stream lies in device memory behind a 256-byte boundary at the residue that gives the row's a0, between guard spans; the
output lies between guard spans over a 0x3C pre-fill. The decoded bytes are the oracle's, the guards are untouched, decode_stats() says
that the parallel kernels took every chunk's regular stream (and its sections where it has any) and decode_trace()["reg_end"] of every
chunk is the piece model's regular-stream end. Byte parity cannot see a chunk the point kernel gives up on -- the kernels behind it
produce the same bytes -- and for a schema without sections neither can the stats or reg_end: k_decode_varint redoes the chunk under
the same status word. So every row without sections runs a second time as its PINNED TWIN (points_token_cases.pinned: the same token
stream, byte for byte, in front of one small Palette section), where sec_done == 2 is the mark only the point kernel's fold leaves
and a handed-back chunk shows sec_done == 1. A second call on the same codec gives the same."""
import numpy as np
import pytest

import points_token_cases as PC

pytestmark = pytest.mark.gpu

FILL, GUARD, SPAN = 0x3C, 0xA7, 256
SHAPES = (1, 2, 16)          # cldn_hip_debug_decode_split: the chained launch, 2 and 16 workgroups per chunk
_prepared = {}
_codecs = {}


def _prep(oracle, row, a0):
    """(streams, ns, the oracle's decode of the batch, one Model per chunk) -- once per (row, a0). A pinned twin: its regular streams
    are the base row's payloads."""
    key = (row.name, row.schema, a0)
    if key not in _prepared:
        streams, ns, _clouds = row.streams(oracle, a0)
        want = np.concatenate([oracle.decode_stage1(row.info(n), s, n, fill=FILL) for s, n in zip(streams, ns)])
        M = row.models(streams, ns, a0)
        if row.base is not None:
            assert PC.carries_the_base_tokens(M, _prep(oracle, row.base, a0)[3])
        _prepared[key] = (streams, ns, want, M)
    return _prepared[key]


def _codec(row, fresh=False):
    """Schemas without sections keep no hints between calls: one codec per schema serves every row. Others get their own."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    if row.sections or fresh:
        return native.Codec(native.Plan(row.info(1)), device=0, stream=torch.cuda.current_stream(dev).cuda_stream), True
    if row.schema not in _codecs:
        _codecs[row.schema] = native.Codec(native.Plan(row.info(1)), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    return _codecs[row.schema], False


def _first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return int(d[0]) if d.size else -1


def _decode(codec, row, prep, a0, out_residue=0, zero_fill=False):
    """One device-resident decode call of the row's batch. Returns (stats, trace) after checking bytes and guards."""
    import torch
    dev = torch.device("cuda", 0)
    streams, ns, want, M = prep
    data = np.concatenate(streams)
    r = (a0 - 4) % 16
    buf = np.full(SPAN + r + data.size + SPAN, 0xEE, dtype=np.uint8)
    buf[SPAN + r:SPAN + r + data.size] = data
    d_stream = torch.from_numpy(buf).to(dev)
    total = sum(ns) * row.step
    obuf = np.full(SPAN + out_residue + total + SPAN, GUARD, dtype=np.uint8)
    obuf[SPAN + out_residue:SPAN + out_residue + total] = FILL
    d_out = torch.from_numpy(obuf).to(dev)
    assert d_stream.data_ptr() % 256 == 0 and d_out.data_ptr() % 256 == 0
    assert (d_stream.data_ptr() + SPAN + r + 4) % 16 == a0
    offs = np.concatenate([[0], np.cumsum([s.size for s in streams])]).astype(np.uint64)
    from cloudini_amd import native
    try:
        codec.decode_device(d_stream.data_ptr() + SPAN + r, offs, np.array(ns, dtype=np.uint64), d_out.data_ptr() + SPAN + out_residue, total, 0)
        codec.status()
    except native.CloudiniHipError as e:
        if e.code == -4:      # CLDN_HIP_ERR_DEVICE, a HIP runtime error: nothing more is started on a device that has faulted
            pytest.exit("%s (a0 %d): HIP error in the decode call: %s" % (row.name, a0, e), returncode=3)
        raise                 # a status of the codec (a well-formed stream called malformed, ...): this row's failure
    stats, tr = codec.decode_stats(), codec.decode_trace()
    got = d_out.cpu().numpy()
    assert np.all(got[:SPAN + out_residue] == GUARD) and np.all(got[SPAN + out_residue + total:] == GUARD), "a guard span was written"
    body = got[SPAN + out_residue:SPAN + out_residue + total]
    if zero_fill:      # set_decode_fill(True): bytes no field covers may be written as 0
        covered = np.zeros(row.step, dtype=bool)
        for f in row.fields:
            covered[f[1]:f[1] + np.dtype(PC.cases._NP[f[2]]).itemsize] = True
        mask = np.tile(covered, sum(ns))
        assert np.all((body[~mask] == 0) | (body[~mask] == FILL))
        body, want = body[mask], want[mask]
    assert np.array_equal(body, want), ("first difference at byte %d" % _first_diff(body, want), stats, tr["reg_end"].tolist())
    return stats, tr


def _check_route_taken(row, M, stats, tr, what):
    want_stats, want_ends = row.expect(M)
    seen = (stats, tr["n_chunks"], tr["reg_end"].tolist())
    assert stats == want_stats, (what, seen)
    assert tr["n_chunks"] == len(M) and tr["reg_end"].tolist() == want_ends, (what, seen, want_ends)
    # one or two integer fields (kFastPalFields): the point kernel folds them, from columns or from their Palettes, and only that
    # fold leaves sec_done == 2. (More fields: whether the column kernels in front delivered is their business, not this grid's.)
    if 1 <= len(PC.int_fields(row.schema)) <= 2:
        assert tr["sec_done"].tolist() == [2] * len(M), (what, tr["sec_done"].tolist())


def _set_split(codec, parts):
    from cloudini_amd import native
    assert codec.decode_split(parts) == 0


def _as_itself_and_pinned(row):
    return [row] if row.sections else [row, PC.pinned(row)]


@pytest.mark.parametrize("row", PC.WELL_FORMED, ids=[r.name for r in PC.WELL_FORMED])
def test_decode(oracle, row):
    a0 = row.a0s[0]
    for run in _as_itself_and_pinned(row):
        prep = _prep(oracle, run, a0)
        for parts in SHAPES:
            codec, mine = _codec(run)
            _set_split(codec, parts)
            for call in range(2):
                stats, tr = _decode(codec, run, prep, a0)
                _check_route_taken(run, prep[3], stats, tr, (run.schema, parts, call))
            if mine:
                codec.close()


RESIDUE_ROWS = PC.SUBSET + PC.FIRST_PIECE


@pytest.mark.parametrize("row", RESIDUE_ROWS, ids=[r.name for r in RESIDUE_ROWS])
def test_decode_at_every_residue(oracle, row):
    """The stream pointer at all 16 residues of a device address and the output pointer at a permutation of them, the row rebuilt for
    each a0 so that its predicate still holds (the CPU test has proven that). The first-piece rows exist once per a0: each runs at its
    own, with the output at the permuted residue. The launch shape is the call's own choice (a SPLIT launch: few chunks)."""
    for run in _as_itself_and_pinned(row):
        codec, mine = _codec(run)
        _set_split(codec, 0)
        for a0 in (row.a0s if row in PC.FIRST_PIECE else range(16)):
            prep = _prep(oracle, run, a0)
            r = (a0 - 4) % 16
            stats, tr = _decode(codec, run, prep, a0, out_residue=(7 * r + 3) % 16)
            _check_route_taken(run, prep[3], stats, tr, (run.schema, a0))
        if mine:
            codec.close()


# kPointsVariants (stage1_decode_route.h) -> the schema and call facts that select it
VARIANTS = {
    (3, 0, 1): ("XYZ", {}),
    (3, 1, 1): ("XYZ_U16", {}),
    (3, 1, 2): ("XYZ_U16", {"fill_zero": 1}),
    (3, 0, 0): ("XYZ_ODD", {}),
    (3, 1, 0): ("XYZ_U16_ODD", {}),
    (3, 2, 0): ("XYZ_2U16", {}),
    (3, 8, 0): ("XYZ_5INTS", {}),
    (4, 0, 0): ("XYZW", {}),
    (4, 1, 0): ("XYZW_U16", {}),
    (4, 2, 0): ("XYZW_2U16", {}),
    (4, 8, 0): ("XYZW_5INTS", {}),
}
VARIANT_ROWS = [r for r in PC.SUBSET if r.family != "regend"]      # (the regular-end rows are rows of their own two schemas)


@pytest.fixture(scope="module")
def route_shim(tmp_path_factory):
    import test_decode_route as TR
    return TR, TR.build_shim(tmp_path_factory.mktemp("points_route"))


def _selected_variant(route_shim, row, n_chunks, call, out_residue):
    """(nops, nf, sm) that decode_route() selects for the row's plan and this call, through the shim of tests/test_decode_route.py.
    The DecodeFacts are that file's restatement (abi_facts) of what decode_framed fills in, with `aligned` taken from the output
    pointer this test really passes; it is not read back from the codec, so a decode_framed that filled the facts differently would
    go unnoticed here -- tools/decode_route_trace.py holds the two together on kernel traces."""
    TR, lib = route_shim
    ops = [(TR.QF32, 4, f[1]) for f in row.fields[:row.nops]]
    adaptive = [(np.dtype(PC.cases._NP[f[2]]).itemsize, f[1]) for f in row.fields[row.nops:]]
    r = TR.row(row.schema, None, row.step, ops, adaptive, v5=1 if adaptive else 0, n_chunks=n_chunks, sized=0,
               aligned=1 if out_residue % 16 == 0 else 0, **call)
    kernels, got = TR.route_of(lib, r)
    assert got["regular"] == "points" and "k_decode_points_w" in kernels
    return got["nops"], got["nf"], got["sm"]


@pytest.mark.parametrize("variant", sorted(VARIANTS), ids=["nops%d_nf%d_sm%d" % v for v in sorted(VARIANTS)])
def test_every_points_variant(oracle, route_shim, variant):
    """The subset's token streams through each entry of kPointsVariants: the same token codes under the schema that selects the
    variant -- asserted through decode_route() itself -- with integer fields that make small Palettes (NF 1, 2) or columns (NF 8)."""
    import test_decode_route as TR
    assert set(VARIANTS) == TR.POINTS_VARIANTS
    schema, call = VARIANTS[variant]
    rows = [r for r in VARIANT_ROWS if r.nops == variant[0]]
    assert len(rows) >= 7
    for base in rows:
        row = PC.Row(base.name, base.family, schema, base.build, base.pred, base.a0s, ints=PC.columns_not_palettes if variant[1] == 8 else None)
        codec, _mine = _codec(row, fresh=True)
        if call.get("fill_zero"):
            codec.set_decode_fill(True)
        _set_split(codec, 0)
        for res in (0, 5, 15):
            a0 = (res + 4) % 16
            prep, base_prep = _prep(oracle, row, a0), _prep(oracle, base, a0)
            # the row's tokens, byte for byte, whatever follows them: its predicate holds on them (facts about the payload's end
            # belong to the row's own schema)
            assert base.pred(base_prep[3], a0) and PC.plain(prep[3], a0)
            assert prep[3][0].a0 == a0 and len(prep[3]) == len(base_prep[3])      # (later chunks of a batch move with the sections' sizes)
            assert all(np.array_equal(m.payload[:m.reg_end], b.payload) for m, b in zip(prep[3], base_prep[3]))
            assert _selected_variant(route_shim, row, len(prep[3]), call, out_residue=0) == variant, (base.name, res)
            stats, tr = _decode(codec, row, prep, a0, zero_fill=bool(call.get("fill_zero")))
            _check_route_taken(row, prep[3], stats, tr, (base.name, res))
        codec.close()


@pytest.mark.parametrize("row", PC.HANDBACK, ids=[r.name for r in PC.HANDBACK])
def test_handed_back(oracle, row):
    """Well-formed chunks with one 5-byte token: the point kernel hands them back, the redo route decodes them -- the oracle's bytes
    and the stats, reg_end and sec_done that the row states (read from the code: points_token_cases._handback_rows, PINNED_REDO_REPORTS).
    As itself the row reports what a kept chunk reports; as its pinned twin the hand-back is seen: sec_done == 1, not 2. The codec
    decodes a row of the grid correctly afterwards."""
    a0 = row.a0s[0]
    for run in (row, PC.pinned(row)):
        prep = _prep(oracle, run, a0)
        m, = prep[3]
        good = PC.BY_NAME["halo_1_tokens_nops%d" % row.nops]
        good = good if run is row else PC.pinned(good)
        g_prep = _prep(oracle, good, 4)
        want_stats, want_end, want_done = run.reports
        want_end = {"payload size": len(m.payload), "regular end": m.reg_end}[want_end]
        assert want_end == m.reg_end and (want_done is None) == (run is row)
        for parts in SHAPES:
            codec, _mine = _codec(run, fresh=True)
            _set_split(codec, parts)
            for call in range(2):
                stats, tr = _decode(codec, run, prep, a0)
                assert stats == want_stats, (run.schema, parts, call, stats)
                assert tr["reg_end"].tolist() == [want_end], (run.schema, parts, call, tr["reg_end"].tolist())
                if want_done is not None:
                    assert tr["sec_done"].tolist() == [want_done], (run.schema, parts, call, tr["sec_done"].tolist())
            stats, tr = _decode(codec, good, g_prep, 4)
            _check_route_taken(good, g_prep[3], stats, tr, (run.schema, parts))
            codec.close()
