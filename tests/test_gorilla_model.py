"""CPU: tests/gorilla_model.py (the Gorilla codec and the device decoder's hand-over rules, restated) against the oracle, on every row
of tests/gorilla_cases.py -- and the proof that every row is what its name says. The GPU file tests/test_gpu_gorilla.py builds on it."""
import numpy as np
import pytest

import gorilla_cases as GC
import gorilla_model as GM
from oracle.binding import OracleError

IDS = lambda rows: [r.name for r in rows]


def _gorilla_columns(row, decoded):
    """The doubles of a decoded cloud as bit patterns, per Gorilla field."""
    pts = decoded.reshape(-1, row.step)
    off = {f[0]: f[1] for f in row.fields}
    return [np.ascontiguousarray(pts[:, off[g]:off[g] + 8]).view("<u8").reshape(-1) for g in row.gnames]


@pytest.mark.parametrize("row", GC.EXPRESSIBLE, ids=IDS(GC.EXPRESSIBLE))
def test_model_encoder_writes_the_oracles_regular_stream(oracle, row):
    stream = row.stream(oracle)
    chunks = GC.split_chunks(stream)
    assert len(chunks) == len(row.ns)
    for (_off, payload), want in zip(chunks, row.model_payloads()):
        got = payload[:len(want)].tobytes()
        assert got == want, "first difference at byte %d" % next(i for i, (a, b) in enumerate(zip(got + b"\0", want)) if a != b)
        if row.schema != "C":
            assert len(payload) == len(want)      # (schema C: the ring's section lies behind the regular stream)


@pytest.mark.parametrize("row", GC.EXPRESSIBLE, ids=IDS(GC.EXPRESSIBLE))
def test_values_for_round_trips(row):
    """The encoder writes exactly the specified tokens from values_for's bit patterns, and decode_tokens returns them."""
    for c in row.chunks:
        for first, specs in c:
            bits = GM.values_for(specs, first)
            tokens, kinds, _w = GM.encode_trace(bits)
            assert kinds == ["first"] + [s[0] for s in specs]
            assert np.array_equal(GM.decode_tokens(tokens), bits)


@pytest.mark.parametrize("row", GC.WELL_FORMED, ids=IDS(GC.WELL_FORMED))
def test_model_decoder_and_predicate(oracle, row):
    """The oracle accepts the stream (hand-written ones included) and returns the model's values; the row's predicate holds; the
    model sends exactly the rows named so to the serial decoder."""
    stream = row.stream(oracle)
    L = GC.layout(row, stream)
    decoded = oracle.decode_stage1(row.info(), stream, row.n, fill=0x5A)
    cols = _gorilla_columns(row, decoded)
    p0 = 0
    for (P, _s, _r, _pieces), n in zip(L, row.ns):
        for g, col in enumerate(cols):
            assert np.array_equal(P.values[g], col[p0:p0 + n]), (row.name, g)
        p0 += n
    if row.hand is None:
        for g, b in enumerate(row.bits()):
            assert np.array_equal(cols[g], b)
    assert row.pred is not None and row.pred(L), row.name
    if not row.decode:      # (a WIDE layout: not the stream kernel's, the hand-over model says nothing about it)
        return
    assert sum(c[1] for c in L) == row.serial, [c[2] for c in L]
    named = (row.family == "h" and ("_41_changes" in row.name or ("_40_changes" in row.name and "last_point" not in row.name))) or \
        row.name.startswith("j_63_in_a_batch")
    assert (row.serial != 0) == named


@pytest.mark.parametrize("row", GC.MALFORMED, ids=IDS(GC.MALFORMED))
def test_malformed_rows_are_refused_by_oracle_and_model(oracle, row):
    stream = row.stream(oracle)
    with pytest.raises(OracleError):
        oracle.decode_stage1(row.info(), stream, row.n)
    with pytest.raises(GM.GorillaError) as e:
        GC.layout(row, stream)
    assert e.value.kind == row.error


def test_values_for_refuses_what_the_encoder_would_not_write():
    for specs in ([("10", None)],                                  # no window yet
                  [GC.opener(10, 10), ("10", 1 << 44)],            # wider than the window's 44 bits
                  [GC.opener(10, 10), ("10", 0)],                  # a difference of 0 is a repeat
                  [GC.opener(10, 10), GC.opener(10, 10)],          # fits the window in effect: the encoder writes '10'
                  [GC.opener(10, 10), GC.opener(12, 30)],          # the same, inside it
                  [GC.opener(10, 10, 1 << 43)],                    # payload's lowest bit clear: ctz would be larger
                  [GC.opener(40, 30)]):                            # clz + ctz > 63
        with pytest.raises(ValueError):
            GM.values_for(specs)
    assert GM.encode_trace(GM.values_for([GC.opener(32, 3), ("10", 5)]))[2][-1] == (31, 3)   # the clamp


def test_windows_in_front_of_encoder_pieces():
    row = GC.BY_NAME["j_piece_edges_B"]
    bits = row.bits()[0]
    _t, kinds, wins = GM.encode_trace(bits)
    front = GM.windows_in_front(bits, 504)
    assert front[0] is None and front[1] == wins[503] and front[2] == wins[1007] and kinds[504] == "11" and front[1] != wins[504]
