"""The mode sweep's numpy model (tests/mode_model.py) against the oracle, which is itself pinned to the compiled reference:
the probed mode is the oracle's, the four section sizes are what forcing a mode does to the oracle's stream, and the reference
decodes every forced-mode stream to the same points. Every assertion is an equality. No GPU."""
import numpy as np
import pytest

import cases
import mode_cases as MC
import mode_model as M
from oracle.binding import OracleError

FAMILIES = [(n, i, d) for n, i, d in cases.encode_cases(small=True) if M.adaptive_fields(i)]
CRAFTED = list(MC.all_crafted())


def _has_min_delta(v):
    lo = np.iinfo(np.int64).min
    return any(((c - np.concatenate([[0], c[:-1]]).astype(np.int64)) == lo).any() for c in (v[k:k + M.CHUNK] for k in range(0, v.size, M.CHUNK)))


def _check(oracle, info, data, decode=None):
    n = data.size // info.point_step
    fields = M.adaptive_fields(info)
    assert len(fields) == oracle.adaptive_field_count(info) and fields
    rep = M.sweep(info, data, [n])[0]
    base, probed = oracle.encode_stage1(info, data, return_modes=True)
    assert rep["probe_mode"].tolist() == probed.tolist()
    assert oracle.encode_stage1_continued(info, data, probed).tobytes() == base.tobytes()
    # A delta of INT64_MIN is written as the byte 0x00 (encodeVarint64 wraps), which every decoder reads as the NaN marker: the
    # reference cannot read such a DeltaVarint or DeltaRle section back, whoever chose the mode. Sizes are checked all the same.
    unreadable = [_has_min_delta(M.column(info, data, f)[0]) for f in fields]
    readable = np.where(unreadable, 1, probed).astype(np.uint8)
    points = oracle.decode_stage1(info, oracle.encode_stage1_continued(info, data, readable), n)
    for a in range(len(fields)):
        rest = set()
        for m in range(4):
            modes = readable.copy()
            modes[a] = m
            stream = oracle.encode_stage1_continued(info, data, modes)
            rest.add(stream.size - int(rep["bytes"][a, m]))      # the same for every mode: sizes differ as the cells do
            for dec in [lambda: oracle.decode_stage1(info, stream, n)] + ([lambda: decode(info, stream)] if decode else []):
                if unreadable[a] and m in (0, 3):
                    with pytest.raises(OracleError):
                        dec()
                else:
                    assert dec().tobytes() == points.tobytes(), (a, m)
        assert len(rest) == 1, (fields[a].name, rest)
    return rep


def test_there_are_families_and_crafted_cases():
    assert len(FAMILIES) >= 20 and len(CRAFTED) >= 100
    assert {FA for _n, i, _d in FAMILIES for FA in (len(M.adaptive_fields(i)),)} >= {1, 2, 5}


@pytest.mark.parametrize("name,info,data", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_model_against_the_oracle_on_every_family_with_adaptive_fields(oracle, name, info, data):
    _check(oracle, info, data)


@pytest.mark.parametrize("name,info,data,check", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_model_against_the_oracle_on_the_crafted_columns(oracle, name, info, data, check):
    v, _bpv = M.column(info, data, M.adaptive_fields(info)[0])
    assert check(v), name
    rep = _check(oracle, info, data)
    if name.endswith("probe_fooled"):
        probe, best = int(rep["probe_mode"][0]), int(rep["best_mode"][0])
        assert probe != 0 and best != probe                                # Palette, Rle or DeltaRle on the constant prefix
        assert int(rep["bytes"][0, probe]) - int(rep["bytes"][0, best]) > 10000


REF_CASES = [c for c in FAMILIES if c[0] in ("c4_velodyne", "two_floats_then_ints", "ouster_step48", "palette_all_distinct_u32")] + \
    [(c[0], c[1], c[2]) for c in CRAFTED if c[0].split("_", 2)[2] in ("probe_fooled", "run_over_chunk_edge", "int64_wrap_and_min", "unique_17500", "unique_5121", "unique_10241", "skewed_partition", "hash_never_separates_0")]


@pytest.mark.parametrize("name,info,data", REF_CASES, ids=[c[0] for c in REF_CASES])
def test_the_reference_decodes_every_forced_mode_stream(oracle, reflib, name, info, data):
    _check(oracle, info, data, decode=lambda i, s: reflib.decode_noheader(i, s))


def test_model_corner_semantics():
    assert M.section_sizes(np.array([7], np.int64), 2) == [1 + 1, 3 + 2 + 0, 5 + 2 + 1, 5 + 1 + 1]
    # 300 equal values: one Rle run with a two-byte length; DeltaRle has the first delta, then 299 zeros
    assert M.section_sizes(np.full(300, 7, np.int64), 4) == [1 + 300, 3 + 4, 5 + 4 + 2, 5 + (1 + 1) + (1 + 2)]
    lo = np.iinfo(np.int64).min
    assert M._varint64_len(np.array([lo, 0, -1, 63, 64, -64, -65], np.int64)).tolist() == [1, 1, 1, 1, 2, 2, 2]
    assert M.select([5, 5, 5, 5]) == 0 and M.select([5, 4, 4, 4]) == 1 and M.select([5, 5, 4, 4]) == 2 and M.select([5, 5, 5, 4]) == 3
    info, data = cases.int_only(np.arange(10, dtype=np.uint32), cases.F.UINT32)
    rep = M.sweep(info, data, [0, 10])
    assert not rep[0].tobytes().strip(b"\0") and rep.shape == (2, 1) and rep[1, 0]["bytes"][0] == 1 + 10
    assert M.adaptive_fields(cases.make_info([("v", 0, cases.F.UINT32, None)], 4, 1, version=4)) == []
