"""The audit report's numpy model (tests/audit_model.py) on round trips through the oracle: which schema families keep the
promise "the error stays below the resolution", and the exact records of constructed offenders. No GPU."""
import numpy as np
import pytest

import audit_cases as A
import audit_model as M
import cases

# Families that do NOT audit clean under the default limits -- the findings the audit exists to show:
#   five_floats       five +inf in field d: the scalar lossy encoder has no tick count for them (n_class_diff)
#   float_specials*   +-inf, +-3e9 m and +-2147483.648 m at 1 mm: beyond int32 ticks, the FloatN sentinel (n_class_diff, n_over_limit)
#   region_overflow*  stretches of +-2.0e6 m at 1 mm: in range for int32, but a float32 there has an ulp of 0.125 m
#                     (max_abs_err 0.125), and +inf
# Their test: not clean by default; clean on the rows inside the encoders' domain under the bound of the number formats
# (audit_cases.format_bound).
FINDINGS = ("five_floats", "float_specials3", "float_specials4", "region_overflow3", "region_overflow4", "region_overflow3_u16",
            "region_overflow3_u16_unaligned", "region_overflow4_unaligned")

CASES = cases.encode_cases(small=True)


def _round_trip(oracle, info, data):
    n = data.size // info.point_step
    return oracle.decode_stage1(info, oracle.encode_stage1(info, data), n)


@pytest.mark.parametrize("name,info,data", CASES, ids=[c[0] for c in CASES])
def test_round_trip_audits_clean_under_default_limits(oracle, name, info, data):
    n = data.size // info.point_step
    dec = _round_trip(oracle, info, data)
    rep = M.audit(info, data, dec, [n])
    print(name, [(f.name, tuple(rep[0, k])) for k, f in enumerate(info.fields)])
    if name not in FINDINGS:
        assert M.clean(info, rep), name
        assert (rep["max_abs_err"][0] <= M.default_limits(info)).all()
        return
    assert not M.clean(info, rep), name
    rows = A.safe_rows(info, data)
    assert 0 < rows.sum() < n
    a, b = A.take_rows(data, info.point_step, rows), A.take_rows(dec, info.point_step, rows)
    inside = M.audit(info, a, b, [int(rows.sum())], A.format_bound(info, a))
    print(name, "inside the domain:", [(f.name, tuple(inside[0, k])) for k, f in enumerate(info.fields)])
    assert M.clean(info, inside), name


def test_constructed_offenders_give_exact_records(oracle):
    info, clouds = A.offender_batch()
    sizes = [c.size // 16 for c in clouds]
    dec = [_round_trip(oracle, info, c) for c in clouds]
    rep = M.audit(info, np.concatenate(clouds), np.concatenate(dec), sizes)
    x, y, z, inten = 0, 1, 2, 3
    # x = 3.0e6 m at 1 mm: 3e9 ticks do not fit int32; both sides finite, so it is an error over the limit, not a class change
    assert (rep[0, x]["n_class_diff"], rep[0, x]["n_over_limit"], rep[0, x]["first_bad_point"]) == (0, 1, 5)
    assert rep[0, x]["max_abs_err"] > 1.0e5
    # +inf: the decode is finite
    assert (rep[1, y]["n_class_diff"], rep[1, y]["n_over_limit"], rep[1, y]["first_bad_point"]) == (1, 0, 7)
    assert rep[1, y]["max_abs_err"] <= 0.001
    # every other record is clean, the neighbours of the two points included
    for k in range(3):
        for f in range(4):
            if (k, f) in ((0, x), (1, y)):
                continue
            r = rep[k, f]
            assert (r["n_class_diff"], r["n_over_limit"], r["first_bad_point"]) == (0, 0, M.NONE), (k, f)
        assert rep[k, inten]["n_bitwise_diff"] == 0
    assert not M.clean(info, rep)

    a, b = A.damage_decoded(clouds)   # audit_clouds only: a NaN on the input side alone, one integer changed
    rep = M.audit(info, np.concatenate(a), np.concatenate(b), sizes)
    assert tuple(rep[1, z]) == (1, 1, 0, 9, 0.0)
    assert tuple(rep[2, inten]) == (1, 0, 0, 11, 0.0)
    assert tuple(rep[1, y]) == (0, 0, 0, M.NONE, 0.0)      # both +inf, same bits: nothing
    for k in range(3):
        for f in range(4):
            if (k, f) not in ((1, z), (2, inten)):
                assert tuple(rep[k, f]) == (0, 0, 0, M.NONE, 0.0), (k, f)


def test_model_corner_semantics():
    """Both sides NaN with different payloads: bitwise only. -0.0 against 0.0: bitwise, and bad only at limit 0. Padding bytes
    and zero-point clouds are never looked at."""
    info = cases.make_info([("v", 1, cases.F.FLOAT32, 0.5), ("k", 6, cases.F.UINT8, None)], 9, 4)
    a = np.full(4 * 9, 0xA5, np.uint8)
    b = np.full(4 * 9, 0x5A, np.uint8)
    va = np.array([0x7fc00000, 0x80000000, 0x3f800000, 0x7f800000], dtype="<u4")   # NaN, -0.0, 1.0, +inf
    vb = np.array([0x7fc00001, 0x00000000, 0x3fc00000, 0xff800000], dtype="<u4")   # NaN', 0.0, 1.5, -inf
    for i in range(4):
        a[i * 9 + 1:i * 9 + 5] = va[i:i + 1].view(np.uint8)
        b[i * 9 + 1:i * 9 + 5] = vb[i:i + 1].view(np.uint8)
        a[i * 9 + 6] = b[i * 9 + 6] = i
    rep = M.audit(info, a, b, [0, 4, 0])
    assert tuple(rep[1, 0]) == (4, 1, 0, 3, 0.5) and tuple(rep[1, 1]) == (0, 0, 0, M.NONE, 0.0)
    assert tuple(rep[0, 0]) == tuple(rep[2, 0]) == (0, 0, 0, M.NONE, 0.0)
    rep = M.audit(info, a, b, [0, 4, 0], [0.0, 0.0])
    assert tuple(rep[1, 0]) == (4, 1, 1, 0, 0.5)
    rep = M.audit(info, a, b, [2, 2], [0.25, 0.0])
    assert tuple(rep[0, 0]) == (2, 0, 0, M.NONE, 0.0) and tuple(rep[1, 0]) == (2, 1, 1, 0, 0.5)
