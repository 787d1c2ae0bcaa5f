"""The call plans of tests/stream_order_cases.py hold what they were built for -- from the plans and the oracle alone, no GPU."""
import numpy as np
import pytest

import cases
import lz4_body
import stream_order_cases as S
from cloudini_amd.schema import FieldType as F
from oracle.binding import OracleError


def _shapes(plan):
    return [S.shape_of(c) for c in plan]


def test_main_plan_shapes():
    shapes = _shapes(S.MAIN_PLAN)
    assert len(shapes) >= 18                                    # the hint is refreshed with every 16th call
    a, b = S.SAME_PAIR
    assert b == a + 1 and shapes[a] == shapes[b]
    for k in range(1, len(shapes)):
        assert (shapes[k] != shapes[k - 1]) or (k - 1, k) == S.SAME_PAIR, k
    # the designed pair: the same shape, other data
    for x, y in zip(S.clouds_of(S.MAIN_PLAN[a]), S.clouds_of(S.MAIN_PLAN[b])):
        assert x.size == y.size and not np.array_equal(x, y)
    # A, B, A: a shape returns that is not the last one
    p, q, r = S.ABA
    assert p < q < r and shapes[p] == shapes[r] != shapes[q] and shapes[r - 1] != shapes[r]
    for want in ([300], [33000, 5], [70001, 0, 1], [4097], [32768], [300] * 9):
        assert want in shapes, want
    assert all(n <= 70001 for s in shapes for n in s)
    # [70001, 0, 1] comes behind smaller calls: more points and more chunks than any call before it
    g = S.GROW_CALL
    assert shapes[g] == [70001, 0, 1] and g > 0
    assert all(sum(s) < sum(shapes[g]) and S.n_chunks_of(s) < S.n_chunks_of(shapes[g]) for s in shapes[:g])
    # k_finish's 200-chunk edge is crossed once, by one-chunk clouds of a few points
    many = [k for k, s in enumerate(shapes) if S.n_chunks_of(s) >= 200]
    assert many == [S.MANY_CHUNKS_CALL]
    assert len(shapes[many[0]]) >= 200 and all(1 <= n <= 16 for n in shapes[many[0]])
    assert all(S.n_chunks_of(s) < 200 for k, s in enumerate(shapes) if k != many[0])


def test_main_plan_commits_the_designed_modes(oracle):
    per_call = []
    for k, call in enumerate(S.MAIN_PLAN):
        want = S.want_encode(oracle, S.INFO, S.clouds_of(call))
        assert want.modes.shape == (len(call), 1)
        for j, m in enumerate(S.designed_modes(call)):
            if m is not None:
                assert int(want.modes[j, 0]) == m, (k, j)
        per_call.append(sorted({int(m) for m in S.designed_modes(call) if m is not None}))
    assert all(len(p) == 1 for k, p in enumerate(per_call) if k != S.MANY_CHUNKS_CALL)
    seq = [p[0] for p in per_call if p]
    # each of the four modes in turn, within the first four calls and again behind the refresh of the hint
    assert sorted(seq[:4]) == [0, 1, 2, 3] and set(seq[16:]) >= {0, 1, 2, 3} - {seq[15]}
    changes = sum(1 for a, b in zip(seq[:-1], seq[1:]) if a != b)
    assert changes >= len(seq) - 2                              # the committed mode changes between all but at most one pair
    # the pair with the same shape changes the mode as well: the hint of the first is wrong for the second
    a, b = S.SAME_PAIR
    assert per_call[a] != per_call[b]


def test_decoys_are_other_valid_inputs_of_the_same_size(oracle):
    differ = 0
    for k, call in enumerate(S.MAIN_PLAN):
        clouds, decoys = S.clouds_of(call), S.decoys_of(call)
        assert [c.size for c in clouds] == [d.size for d in decoys]
        w, d = S.want_encode(oracle, S.INFO, clouds), S.want_encode(oracle, S.INFO, decoys)
        if sum(S.shape_of(call)):
            assert not np.array_equal(w.bytes, d.bytes), k      # a call that read the decoy shows in the bytes
        differ += int(not np.array_equal(w.modes, d.modes))
    assert differ >= len(S.MAIN_PLAN) - 2                       # ... and, for most calls, in the modes


@pytest.mark.parametrize("plan,least", [(S.DECODE_PLAN, 10), (S.STAGE2_DECODE_PLAN, 6), (S.STAGE2_PLAN, 6), (S.ROUND_TRIP_PLAN, 12),
                                        (S.TWO_THREAD_PLAN, 8)])
def test_shorter_plans(plan, least):
    shapes = _shapes(plan)
    assert len(shapes) >= least
    same = [k for k in range(1, len(shapes)) if shapes[k] == shapes[k - 1]]
    assert same == ([] if plan is not S.ROUND_TRIP_PLAN and plan is not S.TWO_THREAD_PLAN else [S.SAME_PAIR[1]])
    assert any(S.n_chunks_of(s) > 1 for s in shapes) and any(len(s) > 1 for s in shapes) and any(0 in s for s in shapes)


def _check_pair(oracle, info, cloud, wrap=None, unwrap=None):
    true, decoy, dcloud = S.decode_pair(oracle, info, cloud, wrap)
    n = cloud.size // info.point_step
    assert true.size == decoy.size
    if n == 0:
        return
    assert not np.array_equal(true, decoy)
    s1_true, s1_decoy = oracle.encode_stage1(info, cloud), oracle.encode_stage1(info, dcloud)
    if wrap is None:
        assert np.array_equal(true, s1_true) and np.array_equal(decoy, s1_decoy)
        assert [p.size for p in S.chunk_payloads(true)] == [p.size for p in S.chunk_payloads(decoy)]
    else:
        assert np.array_equal(unwrap(true), s1_true) and np.array_equal(unwrap(decoy), s1_decoy)
    a, b = oracle.decode_stage1(info, s1_true, n, fill=0), oracle.decode_stage1(info, s1_decoy, n, fill=0)
    assert not np.array_equal(a, b)                            # the decoy is valid and decodes to other points


def test_decode_decoys_have_the_length_of_the_true_streams(oracle):
    for call in S.DECODE_PLAN:
        for cloud in S.clouds_of(call):
            _check_pair(oracle, S.INFO, cloud)
    # the ring of 4 staging buffers comes round: more than 4 calls whose tables are uploaded
    assert sum(1 for call in S.DECODE_PLAN if len(call) >= S.RING_CLOUDS) > 4


def _lz4_unwrap(body):
    import lz4_block_rules as R
    return lz4_body.frame([R.lz4_decompress_safe(c.tobytes(), 1 << 21) for c in S.chunk_payloads(body)])


def _zstd_unwrap(body):
    import zstd_decode_cases as K
    return lz4_body.frame([K.libzstd_decompress(c.tobytes(), 1 << 21) for c in S.chunk_payloads(body)])


def test_stage2_decode_decoys(oracle):
    """host-library bodies: [u32 size][LZ4 block] and [u32 size][ZSTD frame] per chunk, true and decoy of one length"""
    for call in S.STAGE2_DECODE_PLAN:
        for cloud in S.clouds_of(call):
            _check_pair(oracle, S.INFO, cloud, S.lz4_body_of, _lz4_unwrap)
            _check_pair(oracle, S.INFO, cloud, S.zstd_body_of, _zstd_unwrap)


def test_the_other_schemas(oracle):
    info, calls, decoys = S.ouster_calls()
    assert any(int(f.type) == int(F.FLOAT64) and f.resolution is None for f in info.fields)    # a Gorilla field
    assert all(sum(c.size for c in call) // info.point_step <= 5000 for call in calls)
    winfo, wcalls, wdecoys = S.wide_calls()
    assert S.WIDE_SEED in cases.VERY_WIDE_SEEDS and len(winfo.fields) > 64
    assert all(sum(c.size for c in call) // winfo.point_step <= 4097 for call in wcalls)
    for inf, cs, ds in ((info, calls, decoys), (winfo, wcalls, wdecoys)):
        shapes = [[c.size // inf.point_step for c in call] for call in cs]
        assert all(a != b for a, b in zip(shapes[:-1], shapes[1:]))
        for call, dcall in zip(cs, ds):
            assert [c.size for c in call] == [d.size for d in dcall]
            assert not np.array_equal(S.want_encode(oracle, inf, call).bytes, S.want_encode(oracle, inf, dcall).bytes)
            for cloud in call:
                _check_pair(oracle, inf, cloud)


def test_unframed_cases(oracle):
    assert S.UNFRAMED_INFO.version == 3 and not oracle.uses_v5(S.UNFRAMED_INFO)
    for n in S.UNFRAMED_N:
        payload, decoy, cloud = S.unframed_case(oracle, n)
        assert payload.size == decoy.size and not np.array_equal(payload, decoy)
        framed = oracle.encode_stage1(S.UNFRAMED_INFO, cloud)
        assert int.from_bytes(framed[:4].tobytes(), "little") == payload.size and np.array_equal(framed[4:], payload)


def test_the_damaged_stream_is_refused_by_the_oracle(oracle):
    stream, n = S.chunk_missing(oracle)
    with pytest.raises(OracleError):
        oracle.decode_stage1(S.INFO, stream, n)
    assert len(S.chunk_payloads(stream)) == 1 and n > S.CHUNK


def test_device_memory_of_a_run_stays_under_one_gib(oracle):
    """per call: input, decoy source, output with the oracle's bound, offsets, sizes, modes, and a snapshot of every output"""
    total = 0
    for call in S.MAIN_PLAN:
        counts = S.shape_of(call)
        inp = sum(counts) * 16
        out = sum(oracle.stage1_bound(S.INFO, n) for n in counts)
        total += 2 * inp + 2 * (out + 8 * (len(counts) + 1) + 4 * S.n_chunks_of(counts) + len(counts) + 4 * 1024)
    assert total * 2 < 1 << 30          # (twice: the round trip decodes every call as well)
