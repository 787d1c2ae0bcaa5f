"""GPU: k_decode_stream_w (MODE 0 with MSB ends, with the marker kernels' bitmap and in section mode; MODE 1) and k_decode_fixed
(stage1_decode_stream.h) on the constructed grid of tests/stream_token_cases.py, one test per row so that a failure names it.
tests/test_stream_token_cases.py (CPU) proves that every row, and every row's pinned twin, is what it says at every address residue
used here.

Per row and residue: the stream lies in device memory behind a 256-byte boundary at the residue that gives the row's a0, between guard
spans; the output lies between guard spans over a 0x3C pre-fill. The decoded bytes are the oracle's, the guards are untouched,
decode_trace()["reg_end"] of every chunk is the piece model's regular-stream end, and the observable of the row's route says that the
stream kernel kept every chunk (stream_token_cases' docstring: which one, and where it is read from). On the plain `stream` route no
observable tells a kept chunk from one k_decode_varint redid, so every such row runs a second time as its PINNED TWIN on the
`stream_cols` route, where sec_done == 2 is the mark only the stream kernel's column merge leaves. A second call on the same codec
gives the same. Rows whose schema leaves bytes uncovered run with set_decode_fill(True) as well."""
import numpy as np
import pytest

import stream_token_cases as SC

pytestmark = pytest.mark.gpu

FILL, GUARD, SPAN = 0x3C, 0xA7, 256
_prepared = {}
_codecs = {}
_routes = {}


def _prep(oracle, row, a0):
    """(streams, ns, the oracle's decode of the batch, one Model per chunk) -- once per (row, schema, a0)"""
    key = (row.name, row.schema.name, a0)
    if key not in _prepared:
        streams, ns, _clouds = row.streams(oracle, a0)
        want = np.concatenate([oracle.decode_stage1(row.info(n), s, n, fill=FILL) for s, n in zip(streams, ns)])
        M = row.models(streams, ns, a0)
        assert row.pred(M, a0)
        if row.base is not None:
            assert SC.carries_the_base_tokens(M, _prep(oracle, row.base, a0)[3])
        _prepared[key] = (streams, ns, want, M)
    return _prepared[key]


def _codec(row, fill_zero=False):
    """Schemas without sections keep no hints between calls: one codec per (schema, fill) serves every row. Others get their own."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    key = (row.schema.name, fill_zero)
    if row.sections or key not in _codecs:
        codec = native.Codec(native.Plan(row.info(1)), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
        if fill_zero:
            codec.set_decode_fill(True)
        if row.sections:
            return codec, True
        _codecs[key] = codec
    return _codecs[key], False


def _first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return int(d[0]) if d.size else -1


def _decode(codec, row, prep, a0, out_residue=0, zero_fill=False):
    """One device-resident decode call of the row's batch. Returns (stats, trace) after checking bytes and guards."""
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    streams, ns, want, _M = prep
    S = row.schema
    data = np.concatenate(streams)
    r = (a0 - 4) % 16
    buf = np.full(SPAN + r + data.size + SPAN, 0xEE, dtype=np.uint8)
    buf[SPAN + r:SPAN + r + data.size] = data
    d_stream = torch.from_numpy(buf).to(dev)
    total = sum(ns) * S.step
    obuf = np.full(SPAN + out_residue + total + SPAN, GUARD, dtype=np.uint8)
    obuf[SPAN + out_residue:SPAN + out_residue + total] = FILL
    d_out = torch.from_numpy(obuf).to(dev)
    assert d_stream.data_ptr() % 256 == 0 and d_out.data_ptr() % 256 == 0
    assert (d_stream.data_ptr() + SPAN + r + 4) % 16 == a0
    offs = np.concatenate([[0], np.cumsum([s.size for s in streams])]).astype(np.uint64)
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
        covered = np.zeros(S.step, dtype=bool)
        for f in S.fields:
            covered[f[1]:f[1] + SC._SIZE[f[2]]] = True
        mask = np.tile(covered, sum(ns))
        assert np.all((body[~mask] == 0) | (body[~mask] == FILL))
        body, want = body[mask], want[mask]
    assert np.array_equal(body, want), ("first difference at byte %d" % _first_diff(body, want), stats, tr["reg_end"].tolist())
    return stats, tr


def _check_kept(row, M, stats, tr, what):
    """the route's observable of "the stream kernel kept every chunk" (stream_token_cases' docstring)"""
    c, S = len(M), row.schema
    seen = (what, stats, tr["n_chunks"], tr["reg_end"].tolist(), tr["sec_done"].tolist())
    assert tr["n_chunks"] == c and stats[2] == 0 and stats[3] == 0 and stats[0] == c, seen
    assert tr["reg_end"].tolist() == [m.reg_end for m in M], (seen, [m.reg_end for m in M])
    if S.route == "stream_cols":
        assert tr["sec_done"].tolist() == [2] * c and stats[1] == c, seen
    elif S.sections == "side_by_side":
        assert tr["sec_done"].tolist() == [1] * c and stats[1] == c, seen
    else:
        assert stats[1] == 0, seen


@pytest.fixture(scope="module")
def route_shim(tmp_path_factory):
    import test_decode_route as TR
    return TR, TR.build_shim(tmp_path_factory.mktemp("stream_route"))


def _check_route(route_shim, S, n_chunks):
    if (S.name, n_chunks) not in _routes:
        TR, lib = route_shim
        _routes[(S.name, n_chunks)] = SC.check_route(TR, lib, S, n_chunks)


def _runs(row):
    return [row, SC.pinned(row)] if row.schema.name in SC.TWIN else [row]


@pytest.mark.parametrize("row", SC.ROWS, ids=[r.name for r in SC.ROWS])
def test_decode(oracle, route_shim, row):
    for run in _runs(row):
        for fill_zero in ((False, True) if run.schema.padded else (False,)):
            codec, mine = _codec(run, fill_zero)
            for a0 in row.a0s:
                prep = _prep(oracle, run, a0)
                _check_route(route_shim, run.schema, len(prep[3]))
                r = (a0 - 4) % 16
                for call in range(2):
                    stats, tr = _decode(codec, run, prep, a0, out_residue=(7 * r + 3) % 16 if len(row.a0s) > 1 else 0, zero_fill=fill_zero)
                    _check_kept(run, prep[3], stats, tr, (run.schema.name, a0, fill_zero, call))
            if mine:
                codec.close()


def test_no_chunk_is_handed_back_by_design():
    """HANDBACK is empty (stream_token_cases' docstring says why); the longest point the routes admit is in the table"""
    assert SC.HANDBACK == []
    assert "longest_point_begins_at_1023_I64x8" in SC.BY_NAME and SC.SCHEMAS["I64x8"].max_regular == 80 <= SC.MAX_POINT
