"""The resolution sweep's numpy model (tests/sweep_model.py) against the oracle, and against the compiled reference where it is
available: the stream size of a cloud is a sum of per-field terms, and the error a decoder leaves is a function of the point
alone. Every assertion is an equality. No GPU."""
import numpy as np
import pytest

import audit_model as A
import cases
import sweep_model as S
from cloudini_amd import synth

# every field a lossy float: sum of bytes + 4 per chunk == the stream
ABSOLUTE = [("xyzi_struct_4133", cases.xyzi_struct_4133), ("five_floats", cases.five_floats), ("float_specials", cases.float_specials)]

# one lossy float field moved to another resolution: the stream changes by the difference of that field's cells
INCREMENTS = [
    ("mixed_schema", cases.mixed_schema),
    ("header_test_struct_70000", lambda: cases.header_test_struct(70000)),
    ("region_overflow3_u16", lambda: cases.region_overflow(lanes=3, seed=73, with_u16=True)),
    ("float_boundary4", lambda: cases.float_domain_boundary(lanes=4, seed=54)),
    ("float_specials4", lambda: cases.float_specials(lanes=4, seed=4)),
    ("two_floats_then_ints", cases.two_floats_then_ints),
    ("five_floats", cases.five_floats),
    ("depthcam_xyzrgba_320x240", lambda: synth.depthcam_xyzrgba(320, 240)),
]


def _with_resolution(info, f, r):
    out = info.copy()
    out.fields[f].resolution = float(np.float32(r))
    return out


def _zero(cells):
    return not np.ascontiguousarray(cells).view(np.uint8).any()


def _chunks(n):
    return (n + S.CHUNK - 1) // S.CHUNK


def _identities(encode, decode, info, data, absolute):
    """encode(info, data) -> framed stage-1 stream; decode(info, stream, n) -> points. The model against both identities and
    against the audit model of the real round trip, at every rung of the default ladder of every sweepable field."""
    n = data.size // info.point_step
    kinds = S.field_kinds(info)
    ladders = S.default_ladders(info)
    rep = S.sweep(info, data, [n], ladders)[0]
    base = encode(info, data)
    if absolute:
        assert all(k != S.NONE for k in kinds)
        assert int(rep["bytes"][:, 0].sum()) + 4 * _chunks(n) == base.size
    checked = 0
    for f, kind in enumerate(kinds):
        if kind == S.NONE:
            assert _zero(rep[f])
            continue
        for c, r in enumerate(ladders[f]):
            info2 = _with_resolution(info, f, r)
            stream = base if c == 0 else encode(info2, data)
            assert stream.size - base.size == int(rep[f, c]["bytes"]) - int(rep[f, 0]["bytes"]), (info.fields[f].name, float(r))
            audit = A.audit(info2, data, decode(info2, stream, n), [n])[0, f]
            for key in ("n_class_diff", "n_over_limit"):
                assert int(audit[key]) == int(rep[f, c][key]), (info.fields[f].name, float(r), key)
            assert audit["max_abs_err"].tobytes() == rep[f, c]["max_abs_err"].tobytes(), (info.fields[f].name, float(r))
            checked += 1
    assert checked >= 5


@pytest.mark.parametrize("name,make", ABSOLUTE, ids=[c[0] for c in ABSOLUTE])
def test_sum_of_cells_plus_framing_is_the_oracle_stream(oracle, name, make):
    info, data = make()
    _identities(oracle.encode_stage1, oracle.decode_stage1, info, data, absolute=True)


@pytest.mark.parametrize("name,make", INCREMENTS, ids=[c[0] for c in INCREMENTS])
def test_moving_one_field_changes_the_oracle_stream_by_its_cells(oracle, name, make):
    info, data = make()
    if name == "mixed_schema":
        kinds = dict(zip([f.name for f in info.fields], S.field_kinds(info)))
        assert kinds["x"] == kinds["y"] == S.FLOATN and kinds["temp"] == S.SCALAR32 and kinds["stamp"] == S.SCALAR64
    _identities(oracle.encode_stage1, oracle.decode_stage1, info, data, absolute=False)


@pytest.mark.parametrize("name,make", ABSOLUTE + INCREMENTS, ids=[c[0] for c in ABSOLUTE + INCREMENTS])
def test_the_same_against_the_compiled_reference(reflib, name, make):
    info, data = make()

    def decode(info2, stream, n):
        return reflib.decode_noheader(info2, stream)
    _identities(reflib.encode_stage1, decode, info, data, absolute=(name, make) in ABSOLUTE)


def test_field_kinds_follow_the_encoder_selection():
    F = cases.F
    four = [("a", 0, F.FLOAT32, 0.1), ("b", 4, F.FLOAT32, 0.1), ("c", 8, F.FLOAT32, 0.1), ("d", 12, F.FLOAT32, 0.1)]
    assert S.field_kinds(cases.make_info(four, 16, 1)) == [S.FLOATN] * 4
    assert S.field_kinds(cases.make_info(four[:2], 16, 1)) == [S.SCALAR32] * 2
    five = four + [("e", 16, F.FLOAT32, 0.1)]
    assert S.field_kinds(cases.make_info(five, 20, 1)) == [S.SCALAR32] * 5
    mixed = four[:3] + [("k", 12, F.UINT16, None), ("t", 16, F.FLOAT64, 1e-6), ("u", 24, F.FLOAT64, None), ("w", 32, F.FLOAT32, None)]
    assert S.field_kinds(cases.make_info(mixed, 36, 1)) == [S.FLOATN] * 3 + [S.NONE, S.SCALAR64, S.NONE, S.NONE]
    for enc in (cases.EncodingOptions.NONE, cases.EncodingOptions.LOSSLESS):
        assert S.field_kinds(cases.make_info(mixed, 36, 1, enc=enc)) == [S.NONE] * 7


def test_model_corner_semantics():
    """Half ticks: the FloatN group rounds to even, the scalar encoder away from zero. The reference is 0 at a chunk start and
    behind a NaN. +-inf and values beyond the tick range take the sentinel; a skipped rung is a zero cell."""
    v = np.array([0.5, 1.5, 2.5, -0.5, -2.5], dtype=np.float32)
    assert S.decoded(S.FLOATN, v, 1.0).tolist() == [0.0, 2.0, 2.0, -0.0, -2.0]
    assert S.decoded(S.SCALAR32, v, 1.0).tolist() == [1.0, 2.0, 3.0, -1.0, -3.0]
    assert S.decoded(S.SCALAR64, v.astype(np.float64), 1.0).tolist() == [1.0, 2.0, 3.0, -1.0, -3.0]
    # tokens: 100 -> 2 bytes (zig-zag 200 + 1), then deltas of 0 -> 1 byte; a NaN is 1 byte and resets the reference
    v = np.array([100, 100, np.nan, 100, 100], dtype=np.float32)
    for kind in (S.FLOATN, S.SCALAR32):
        assert S.field_cell(kind, v, 1.0) == (2 + 1 + 1 + 2 + 1, 0, 0, 0.0)
    # the reference is 0 again at point 32768
    v = np.full(S.CHUNK + 2, 100, dtype=np.float32)
    assert S.field_cell(S.FLOATN, v, 1.0)[0] == 2 + (S.CHUNK - 1) + 2 + 1
    # sentinels: +inf decodes to a finite value (class), 3e9 m at 1 mm is beyond int32 ticks but finite on both sides (limit)
    v = np.array([np.inf, 3e9, 1.0], dtype=np.float32)
    cell = S.field_cell(S.FLOATN, v, 0.001)
    assert cell[1:3] == (1, 1) and cell[3] > 1e6
    assert S.field_cell(S.SCALAR32, v, 0.001)[1] == 1              # (int64 ticks hold 3e12: no sentinel there)
    info = cases.make_info([("v", 0, cases.F.FLOAT32, 1.0), ("w", 4, cases.F.FLOAT32, 1.0)], 8, 3)
    data = np.arange(6, dtype=np.float32).view(np.uint8)
    rep = S.sweep(info, data, [0, 3], [[1.0, 0.0, 0.5], [0.0, 0.0, 2.0]])
    assert _zero(rep[0]) and _zero(rep[1, :, 1]) and _zero(rep[1, 1, 0])
    assert rep[1, 0, 0]["bytes"] == 3 and rep[1, 0, 2]["bytes"] == 3 and rep[1, 1, 2]["max_abs_err"] == 1.0


@pytest.mark.parametrize("bad", [-0.001, np.nan, np.inf, -np.inf, 1e-45, 2.0e-39])
def test_ladder_rules(bad):
    info, _ = cases.xyzi_struct_4133()
    res = S.default_ladders(info)
    S.check_ladders(info, res)
    res[2, 3] = np.float32(bad)
    with pytest.raises(ValueError):
        S.check_ladders(info, res)
    with pytest.raises(ValueError):
        S.check_ladders(info, np.ones((4, 17), np.float32))
    with pytest.raises(ValueError):
        S.check_ladders(info, np.ones((4, 0), np.float32))
