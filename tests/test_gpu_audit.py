"""Per-field error reports on the device (cloudini_amd/csrc/audit_kernels.hip): cldn_hip_audit_clouds, _streams, _last_encode.

Expected reports never come from the code under test: they are tests/audit_model.py on the same two buffers, and where a
decode is involved the second buffer is the ORACLE's decode of the oracle's streams. Every comparison is exact, record for
record, max_abs_err by its bits."""
import numpy as np
import pytest

import audit_cases as A
import audit_model as M
import cases
import lz4_body as B
from cloudini_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


def _codec(info):
    from cloudini_amd import native
    return native.Codec(native.Plan(info))


def _same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not M.same(got, want):
        bad = [(k, f, tuple(got[k, f]), tuple(want[k, f])) for k in range(got.shape[0]) for f in range(got.shape[1])
               if got[k, f].tobytes() != want[k, f].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} records differ, first (cloud, field, got, want): {bad[:4]}")


def _dev(arr, residue=0, guard=GUARD):
    """A device copy of `arr` that starts `residue` (< 16) bytes behind a 256-byte boundary, between two guard spans. Returns
    (tensor, pointer, check) -- check() asserts that guards and content are as they were."""
    import torch
    dev = torch.device("cuda", 0)
    arr = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.full((256 + guard + 16 + arr.size + guard,), FILL, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + guard + residue
    if arr.size:
        t[base:base + arr.size] = torch.from_numpy(arr.copy()).to(dev)
    before = t.cpu().numpy().copy()

    def check():
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), before), "a buffer the audit may only read has changed"
    return t, t.data_ptr() + base, check


def _dev_report(n_clouds, n_fields):
    """A device report between guard spans, pre-filled; returns (read, pointer): read() checks the guards and returns it."""
    import torch
    dev = torch.device("cuda", 0)
    nbytes = n_clouds * n_fields * 40
    t = torch.full((256 + GUARD + nbytes + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + GUARD
    torch.cuda.synchronize()  # the codec works on a stream of its own: the fill lands before a call writes the report

    def read():
        torch.cuda.synchronize()
        h = t.cpu().numpy()
        assert (h[:base] == 0xEE).all() and (h[base + nbytes:] == 0xEE).all(), "the audit wrote outside its report"
        return h[base:base + nbytes].copy().view(M.DTYPE).reshape(n_clouds, n_fields)
    return read, t.data_ptr() + base


def _round_trip(oracle, info, data):
    return oracle.decode_stage1(info, oracle.encode_stage1(info, data), data.size // info.point_step)


def _perturbed(rs, info, data, n_hits=40):
    """A copy of `data` with a few bytes changed anywhere (field bytes and padding alike)."""
    b = data.copy()
    if b.size:
        at = rs.randint(0, b.size, min(n_hits, b.size))
        b[at] ^= rs.randint(1, 256, at.size).astype(np.uint8)
    return b


# ---- audit_clouds against the model ------------------------------------------------------------------------------------

FAMILIES = cases.encode_cases(small=True) + A.wide_cases()


@pytest.mark.parametrize("name,info,data", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_audit_clouds_equals_the_model_on_every_schema_family(oracle, name, info, data):
    n = data.size // info.point_step
    dec = _round_trip(oracle, info, data)
    codec = _codec(info)
    _same(codec.audit_clouds_host([data], [dec]), M.audit(info, data, dec, [n]), name)
    # the true bound of the number formats as explicit limits, and limit 0 everywhere (first_bad_point then follows the bits)
    for lim in (A.format_bound(info, data), np.zeros(len(info.fields))):
        _same(codec.audit_clouds_host([data], [dec], limit=lim), M.audit(info, data, dec, [n], lim), name)
    # a second cloud whose differences hit padding and integer fields too
    rs = np.random.RandomState(len(name))
    other = _perturbed(rs, info, dec)
    _same(codec.audit_clouds_host([data, dec, data[:0]], [dec, other, data[:0]]),
          M.audit(info, np.concatenate([data, dec]), np.concatenate([dec, other]), [n, n, 0]), name)


@pytest.mark.parametrize("schema", ["xyzi", "step19_odd", "mixed47", "step200"])
def test_ragged_batches_with_zero_point_clouds(oracle, schema):
    rs = np.random.RandomState(3)
    if schema == "xyzi":
        info, base = synth.lidar_xyzi(9000)
    elif schema == "mixed47":
        info, base = cases.mixed_schema(9000)
    else:
        info, base = [(i, d) for nm, i, d in cases.stride_variants() if nm == schema][0]
    step = info.point_step
    sizes = [0, 1, 1023, 0, 1024, 1025, 2048, 0, 3000, 63, 0]
    a, at = [], 0
    for n in sizes:
        a.append(base[at * step:(at + n) * step].copy())
        at += n
    b = [_perturbed(rs, info, c, 25) for c in a]
    codec = _codec(info)
    want = M.audit(info, np.concatenate(a), np.concatenate(b), sizes)
    _same(codec.audit_clouds_host(a, b), want, schema)
    assert (want["n_bitwise_diff"].sum(axis=1)[[0, 3, 7, 10]] == 0).all()
    # all clouds empty, and no cloud at all
    empty = codec.audit_clouds_host([base[:0]] * 3, [base[:0]] * 3)
    _same(empty, M.audit(info, base[:0], base[:0], [0, 0, 0]), schema)
    assert codec.audit_clouds_host([], []).shape == (0, len(info.fields))


@pytest.mark.parametrize("schema", ["xyzi", "step19_odd"])
def test_both_buffers_at_all_16_address_residues(oracle, schema):
    if schema == "xyzi":
        info, data = synth.lidar_xyzi(5000)
    else:
        info, data = [(i, d[:5000 * 19].copy()) for nm, i, d in cases.stride_variants() if nm == schema][0]
    sizes = [1500, 0, 2477, 1023]
    dec = np.concatenate([_round_trip(oracle, info, data[s * info.point_step:e * info.point_step])
                          for s, e in zip(np.cumsum([0] + sizes[:-1]), np.cumsum(sizes))])
    want = M.audit(info, data, dec, sizes)
    codec = _codec(info)
    for ra in range(16):
        rb = (5 * ra + 3) % 16            # a permutation: both buffers see every residue
        _ta, pa, check_a = _dev(data, ra)
        _tb, pb, check_b = _dev(dec, rb)
        read, pr = _dev_report(len(sizes), len(info.fields))
        assert codec.audit_clouds_device(pa, pb, sizes, report_ptr=pr) is None
        _same(read(), want, f"{schema} residues {ra}/{rb}")
        check_a()
        check_b()


def test_host_and_device_locations_in_all_four_combinations(oracle):
    from cloudini_amd import native
    info, data = cases.header_test_struct(5000)
    dec = _round_trip(oracle, info, data)
    sizes = [2000, 3000]
    want = M.audit(info, data, dec, sizes)
    codec = _codec(info)
    _ta, pa, check_a = _dev(data, 4)
    _tb, pb, check_b = _dev(dec, 9)
    for a_loc in (native.HOST, native.DEVICE):
        for b_loc in (native.HOST, native.DEVICE):
            a_ptr = pa if a_loc == native.DEVICE else data.ctypes.data
            b_ptr = pb if b_loc == native.DEVICE else dec.ctypes.data
            _same(codec.audit_clouds_device(a_ptr, b_ptr, sizes, a_loc=a_loc, b_loc=b_loc), want, (a_loc, b_loc))
            read, pr = _dev_report(2, len(info.fields))
            codec.audit_clouds_device(a_ptr, b_ptr, sizes, report_ptr=pr, a_loc=a_loc, b_loc=b_loc)
            _same(read(), want, (a_loc, b_loc, "device report"))
    check_a()
    check_b()


def test_constructed_offenders(oracle):
    info, clouds = A.offender_batch()
    sizes = [c.size // 16 for c in clouds]
    dec = [_round_trip(oracle, info, c) for c in clouds]
    codec = _codec(info)
    got = codec.audit_clouds_host(clouds, dec)
    _same(got, M.audit(info, np.concatenate(clouds), np.concatenate(dec), sizes))
    assert (got[0, 0]["n_class_diff"], got[0, 0]["n_over_limit"], got[0, 0]["first_bad_point"]) == (0, 1, 5)
    assert (got[1, 1]["n_class_diff"], got[1, 1]["n_over_limit"], got[1, 1]["first_bad_point"]) == (1, 0, 7)
    a, b = A.damage_decoded(clouds)
    got = codec.audit_clouds_host(a, b)
    _same(got, M.audit(info, np.concatenate(a), np.concatenate(b), sizes))
    assert tuple(got[1, 2]) == (1, 1, 0, 9, 0.0) and tuple(got[2, 3]) == (1, 0, 0, 11, 0.0)
    # the same through the codec: the streams of the offenders against their points
    streams = [oracle.encode_stage1(info, c) for c in clouds]
    _same(codec.audit_streams_host(clouds, streams), M.audit(info, np.concatenate(clouds), np.concatenate(dec), sizes))


def test_float32_differences_are_taken_in_double():
    """|a - b| of two float32 is not a float32 in general: 16777216 - 0.5 rounds to 16777216 in float32. Limits on either side
    of the exact difference tell the two apart; max_abs_err carries the exact value."""
    info = cases.make_info([("v", 0, cases.F.FLOAT32, 1.0)], 4, 6)
    a = np.array([16777216.0, 16777216.0, 3.0e38, -3.0e38, 1.0e-45, 0.1], dtype="<f4")
    b = np.array([0.5, -0.5, -3.0e38, 3.0e38, -1.0e-45, 0.1], dtype="<f4")
    codec = _codec(info)
    for lim in ([16777215.75], [16777216.25], [6.0e38], [0.0]):
        want = M.audit(info, a.view(np.uint8), b.view(np.uint8), [6], lim)
        _same(codec.audit_clouds_host([a.view(np.uint8)], [b.view(np.uint8)], limit=lim), want, lim)
    want = M.audit(info, a.view(np.uint8), b.view(np.uint8), [6], [16777215.75])
    assert want[0, 0]["n_over_limit"] == 3 and want[0, 0]["max_abs_err"] == 2 * float(np.float32(3.0e38))


def test_32_clouds_of_a_million_points_with_differences_at_block_and_cloud_boundaries():
    import torch
    dev = torch.device("cuda", 0)
    n, n_clouds = 1 << 20, 32
    info, one = synth.lidar_xyzi(n)
    codec = _codec(info)
    d_a = torch.from_numpy(one).to(dev).repeat(n_clouds)
    d_b = d_a.clone()
    rs = np.random.RandomState(9)
    want = np.zeros((n_clouds, 4), dtype=M.DTYPE)
    want["first_bad_point"] = M.NONE
    for cloud in (0, 17, n_clouds - 1):
        b = one.copy()
        for p in (0, 1023, 1024, n - 1):
            f = int(rs.randint(0, 4))
            if f < 3:
                b.view("<f4").reshape(-1, 4)[p, f] += np.float32(0.25 * (1 + p % 3))
            else:
                b.view("<u2").reshape(-1, 8)[p, 6] ^= 1
        d_b[cloud * n * 16:(cloud + 1) * n * 16] = torch.from_numpy(b).to(dev)
        want[cloud] = M.audit(info, one, b, [n])[0]
    assert want["n_over_limit"].sum() + want["n_bitwise_diff"][:, 3].sum() == 12
    read, pr = _dev_report(n_clouds, 4)
    codec.audit_clouds_device(d_a.data_ptr(), d_b.data_ptr(), [n] * n_clouds, report_ptr=pr)
    _same(read(), want)
    # the same batch cut differently: what sat at the start of a cloud is now inside one, the counters only move
    sizes = [27 * n - 1, 1, 5 * n]
    starts = [0, 27 * n - 1, 27 * n]
    got = codec.audit_clouds_device(d_a.data_ptr(), d_b.data_ptr(), sizes)
    assert tuple(got[1, 0]) == (0, 0, 0, M.NONE, 0.0)
    for f in range(4):
        for key in ("n_bitwise_diff", "n_class_diff", "n_over_limit"):
            assert int(got[key][:, f].sum()) == int(want[key][:, f].sum()), (f, key)
        assert got["max_abs_err"][:, f].max() == want["max_abs_err"][:, f].max()
        for j, (lo, hi) in enumerate(zip(starts, starts[1:] + [n * n_clouds])):
            hits = [k * n + int(want[k, f]["first_bad_point"]) for k in range(n_clouds) if want[k, f]["first_bad_point"] != M.NONE]
            hits = [h - lo for h in hits if lo <= h < hi]
            assert int(got[j, f]["first_bad_point"]) == (min(hits) if hits else M.NONE), (j, f)


def _dev_cells(nbytes):
    """A pre-filled device span of `nbytes` between guard spans; returns (read, pointer): read() checks the guards and returns
    the bytes. It does not synchronise."""
    import torch
    t = torch.full((256 + GUARD + nbytes + GUARD,), 0xEE, dtype=torch.uint8, device=torch.device("cuda", 0))
    base = (-t.data_ptr()) % 256 + GUARD

    def read():
        h = t.cpu().numpy()
        assert (h[:base] == 0xEE).all() and (h[base + nbytes:] == 0xEE).all(), "a call wrote outside its report"
        return h[base:base + nbytes].copy()
    return read, t.data_ptr() + base


@pytest.mark.parametrize("schema", ["step19_odd", "step200"])
def test_audit_sweep_and_modes_interleaved_on_one_codec(schema):
    """The three report calls share one table staging buffer, one device table and one event. Audit, sweep, mode sweep and
    the first audit again on one codec, device inputs at address residue 7, device reports, nothing between the calls: the
    tables grow, shrink and grow again (3 clouds / 4 blocks, 1 cloud / 1 block, 5 clouds / 8 units per field, then the first),
    and the shapes cross a block edge (1024), the probe edge (4096) and a chunk edge (32768) by one point."""
    import torch
    import mode_model as MM
    import sweep_model as SM
    info, data = [(i, d) for nm, i, d in cases.stride_variants() if nm == schema][0]
    step, nf, na = info.point_step, len(info.fields), len(MM.adaptive_fields(info))
    assert na == 1
    audit_sizes, sweep_sizes, mode_sizes = [0, 1025, 2049], [1], [1, 0, 4097, 32769, 63]
    a = data[:sum(audit_sizes) * step].copy()
    b = _perturbed(np.random.RandomState(12), info, a, 60)
    pts = data[:sum(mode_sizes) * step].copy()
    ladders = SM.default_ladders(info, (1.0, 0.5))
    want_audit = M.audit(info, a, b, audit_sizes)
    want_sweep = SM.sweep(info, pts[:step], sweep_sizes, ladders)
    want_modes = MM.sweep(info, pts, mode_sizes)
    _ta, pa, check_a = _dev(a, 7)
    _tb, pb, check_b = _dev(b, 7)
    _tp, pp, check_p = _dev(pts, 7)
    read_a1, pr_a1 = _dev_cells(want_audit.nbytes)
    read_s, pr_s = _dev_cells(want_sweep.nbytes)
    read_m, pr_m = _dev_cells(want_modes.nbytes)
    read_a2, pr_a2 = _dev_cells(want_audit.nbytes)
    codec = _codec(info)
    torch.cuda.synchronize()
    assert codec.audit_clouds_device(pa, pb, audit_sizes, report_ptr=pr_a1) is None
    assert codec.sweep_clouds_device(pp, sweep_sizes, ladders, report_ptr=pr_s) is None
    assert codec.sweep_modes_device(pp, mode_sizes, report_ptr=pr_m) is None
    assert codec.audit_clouds_device(pa, pb, audit_sizes, report_ptr=pr_a2) is None
    torch.cuda.synchronize()
    first = read_a1().view(M.DTYPE).reshape(want_audit.shape)
    _same(first, want_audit, schema + " audit")
    assert SM.same(read_s().view(SM.DTYPE).reshape(want_sweep.shape), want_sweep), schema + " sweep"
    assert read_m().tobytes() == np.ascontiguousarray(want_modes).tobytes(), schema + " modes"
    _same(read_a2().view(M.DTYPE).reshape(want_audit.shape), first, schema + " audit again")
    assert want_audit["n_bitwise_diff"].sum() > 0
    check_a()
    check_b()
    check_p()


# ---- audit_streams -----------------------------------------------------------------------------------------------------

STREAM_CASES = ["c2_xyzi", "c4_velodyne", "mixed_v5", "mixed_v4", "ouster_like_gorilla", "five_floats", "float_specials3",
                "region_overflow4", "two_floats_then_ints", "step19_odd", "lossless_f64_padded"]


def _case(name):
    for nm, info, data in FAMILIES:
        if nm == name:
            return info, data
    raise KeyError(name)


@pytest.mark.parametrize("name", STREAM_CASES + ["very_wide_9000"])
def test_audit_streams_equals_the_model_on_points_and_oracle_decode(oracle, name):
    info, data = _case(name)
    step = info.point_step
    n = data.size // step
    cut = [0, n // 3, n // 3, n]                      # three clouds, the middle one empty
    clouds = [data[s * step:e * step] for s, e in zip(cut[:-1], cut[1:])]
    streams = [oracle.encode_stage1(info, c) if c.size else c[:0] for c in clouds]
    dec = [oracle.decode_stage1(info, s, c.size // step) if c.size else c[:0] for s, c in zip(streams, clouds)]
    want = M.audit(info, data, np.concatenate(dec), [c.size // step for c in clouds])
    codec = _codec(info)
    _same(codec.audit_streams_host(clouds, streams), want, name)
    if name != "very_wide_9000":
        bodies = [B.body_of(s) if s.size else s for s in streams]
        _same(codec.audit_streams_host(clouds, bodies, stream_kind=1), want, name + " lz4")
    # device buffers at odd addresses, device report
    _tp, pp, check_p = _dev(data, 5)
    all_streams = np.concatenate(streams)
    _ts, ps, check_s = _dev(all_streams, 11)
    offs = np.concatenate([[0], np.cumsum([s.size for s in streams])])
    read, pr = _dev_report(3, len(info.fields))
    codec.audit_streams_device(pp, ps, offs, [c.size // step for c in clouds], report_ptr=pr)
    _same(read(), want, name + " device")
    check_p()
    check_s()


@pytest.mark.parametrize("kind", [0, 1])
def test_a_damaged_stream_returns_the_decode_error_and_leaves_the_report(oracle, kind):
    from cloudini_amd import native
    info, data = synth.lidar_xyzi(40000)
    stream = oracle.encode_stage1(info, data)
    good = B.body_of(stream) if kind else stream
    codec = _codec(info)
    for what, bad in (("truncated", good[:-7]), ("trailing", np.concatenate([good, np.zeros(3, np.uint8)]))):
        rep = np.zeros((1, 4), dtype=M.DTYPE)
        rep.view(np.uint8)[...] = 0x5C
        with pytest.raises(native.CloudiniHipError) as e:
            codec.audit_streams_host([data], [bad], stream_kind=kind, report=rep)
        assert e.value.code == -6, what
        with pytest.raises(native.CloudiniHipError) as e2:
            (codec.decode_lz4_host if kind else codec.decode_host)([bad], [40000])
        assert e2.value.message == e.value.message
        assert (rep.view(np.uint8) == 0x5C).all(), what
        # and on the device
        _tp, pp, _c = _dev(data)
        _ts, ps, _c2 = _dev(bad)
        read, pr = _dev_report(1, 4)
        with pytest.raises(native.CloudiniHipError):
            codec.audit_streams_device(pp, ps, [0, bad.size], [40000], stream_kind=kind, report_ptr=pr)
        assert (read().view(np.uint8) == 0xEE).all()
    # the codec still works
    _same(codec.audit_streams_host([data], [good], stream_kind=kind),
          M.audit(info, data, oracle.decode_stage1(info, stream, 40000), [40000]))


def test_the_decode_fill_setting_has_no_part_in_the_verdict(oracle):
    info, data = cases.padded_fourth_lane("pcl_xyzi", n=20000)
    stream = oracle.encode_stage1(info, data)
    want = M.audit(info, data, oracle.decode_stage1(info, stream, 20000), [20000])
    codec = _codec(info)
    for zero in (False, True):
        codec.set_decode_fill(zero)
        _same(codec.audit_streams_host([data], [stream]), want)


# ---- audit_last_encode -------------------------------------------------------------------------------------------------

def _batch(info, data, parts=(0.4, 0.0, 0.6)):
    step = info.point_step
    n = data.size // step
    cut = np.concatenate([[0], np.cumsum([int(n * p) for p in parts])])
    return [data[s * step:e * step].copy() for s, e in zip(cut[:-1], cut[1:])]


# (the wide route shares the LZ4 stage: one stage-2 setting is enough for it)
@pytest.mark.parametrize("name,stage2", [(nm, s2) for nm in ("c2_xyzi", "c4_velodyne", "mixed_v5", "float_specials4") for s2 in (0, 1, 2)]
                         + [("very_wide_9000", 0)])
def test_audit_last_encode_after_encode_host(oracle, name, stage2):
    from cloudini_amd import native
    info, data = _case(name)
    clouds = _batch(info, data)
    sizes = [c.size // info.point_step for c in clouds]
    codec = _codec(info)
    codec.set_stage2(stage2)
    streams, _sizes, _modes = codec.encode_host(clouds)
    got = codec.audit_last_encode()
    again = codec.audit_last_encode(limit=np.zeros(len(info.fields)))          # repeatable, other limits
    dec = [_round_trip(oracle, info, c) if c.size else c for c in clouds]
    _same(got, M.audit(info, np.concatenate(clouds), np.concatenate(dec), sizes), name)
    _same(again, M.audit(info, np.concatenate(clouds), np.concatenate(dec), sizes, np.zeros(len(info.fields))), name)
    read, pr = _dev_report(len(clouds), len(info.fields))
    codec.audit_last_encode(report_ptr=pr)
    _same(read(), got, name)
    _same(codec.audit_streams_host(clouds, streams, stream_kind=1 if stage2 else 0), got, name)   # (drops the state)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.audit_last_encode()
    assert e.value.code == -1 and "no encode call to audit" in e.value.message


def test_audit_last_encode_is_refused_without_an_encode_and_after_an_intervening_call(oracle):
    from cloudini_amd import native
    info, data = synth.lidar_xyzi(20000)
    codec = _codec(info)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.audit_last_encode()
    assert e.value.code == -1
    streams, _s, _m = codec.encode_host([data])
    codec.synchronize()
    codec.status()                                    # queries leave the state
    assert codec.audit_last_encode().shape == (1, 4)
    for intervening in (lambda: codec.decode_host(streams, [20000]),
                        lambda: codec.viz_preprocess_host(data, 16, 0, 0.05),
                        lambda: codec.audit_clouds_host([data], [data]),
                        lambda: codec.lz4_decompress_host([b"\x00"], [8])):
        codec.encode_host([data])
        intervening()
        with pytest.raises(native.CloudiniHipError) as e:
            codec.audit_last_encode()
        assert e.value.code == -1 and "no encode call to audit" in e.value.message


@pytest.mark.parametrize("stage2", [0, 1])
@pytest.mark.parametrize("residue", [0, 7])
def test_audit_last_encode_after_encode_device(oracle, stage2, residue):
    import torch
    dev = torch.device("cuda", 0)
    info, data = synth.velodyne_xyzir(60000)
    clouds = _batch(info, data, (0.5, 0.5))
    sizes = [c.size // info.point_step for c in clouds]
    codec = _codec(info)
    codec.set_stage2(stage2)
    cap = sum(codec.plan.stage2_bound(n, stage2) for n in sizes)
    _tp, pp, check_p = _dev(data[:sum(sizes) * info.point_step], residue)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(len(sizes) + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.encode_device(pp, sizes, d_out.data_ptr() + residue, cap, d_off.data_ptr())
    got = codec.audit_last_encode()
    dec = [_round_trip(oracle, info, c) for c in clouds]
    _same(got, M.audit(info, np.concatenate(clouds), np.concatenate(dec), sizes))
    offs = d_off.cpu().numpy().astype(np.uint64)
    _same(codec.audit_streams_device(pp, d_out.data_ptr() + residue, offs, sizes, stream_kind=stage2), got)
    check_p()


def test_audit_last_encode_after_a_framed_chunk_table(oracle):
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, data = synth.lidar_xyzi(70000)
    codec = _codec(info)
    _tp, pp, _check = _dev(data)
    codec.encode_chunks_device(pp, [70000])
    with pytest.raises(native.CloudiniHipError):
        codec.audit_last_encode()                     # not framed yet
    codec.encode_chunks_device(pp, [70000])
    cap = codec.plan.stage1_bound(70000)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.frame_chunks_device(d_out.data_ptr(), cap)
    _same(codec.audit_last_encode(), M.audit(info, data, _round_trip(oracle, info, data), [70000]))


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("stage2", [0, 2])
def test_audit_last_encode_after_encode_viz_judges_the_survivors(oracle, gather, stage2):
    info, data = synth.velodyne_xyzir(50000)
    step = info.point_step
    clouds = _batch(info, data, (0.3, 0.0, 0.7))
    clouds[0].view("<f4")[0] = np.nan                                # dropped by the filter, not an audit finding
    codec = _codec(info)
    codec.set_stage2(stage2)
    streams, _cs, _m, kept = codec.encode_viz(clouds, 0, 0.05, gather=gather)
    got = codec.audit_last_encode()
    survivors = [oracle.viz_preprocess(c, step, 0, 0.05) if c.size else c for c in clouds]
    assert [s.size // step for s in survivors] == [int(k) for k in kept]
    assert 0 < int(kept.sum()) < 50000
    dec = [_round_trip(oracle, info, s) if s.size else s for s in survivors]
    want = M.audit(info, np.concatenate(survivors), np.concatenate(dec), [int(k) for k in kept])
    _same(got, want)
    assert M.clean(info, got)
    _same(codec.audit_streams_host(survivors, streams, stream_kind=1 if stage2 else 0), got)


def test_fetch_output_before_or_after_makes_no_difference(oracle):
    """Two-step host output: the streams wait in the codec's buffer; the audit reads them there and leaves them there."""
    info, data = synth.velodyne_xyzir(50000)
    clouds = _batch(info, data, (0.5, 0.5))
    codec = _codec(info)
    ref_streams, _cs, _m, kept = codec.encode_viz(clouds, 0, 0.05)
    want = codec.audit_last_encode()
    import ctypes as C
    from cloudini_amd import native
    step = info.point_step
    arrs = [c.view(np.uint8).reshape(-1) for c in clouds]
    npts = np.array([a.size // step for a in arrs], dtype=np.uint64)
    offs = np.zeros(3, dtype=np.uint64)
    kept2 = np.zeros(2, dtype=np.uint64)
    cs = np.zeros(8, dtype=np.uint32)
    modes = np.zeros(16, dtype=np.uint8)
    flat = np.concatenate(arrs)
    native._check(native.lib().cldn_hip_encode_stage1_viz(
        codec._h, flat.ctypes.data_as(C.c_void_p), native.HOST, npts.ctypes.data_as(C.POINTER(C.c_uint64)), 2, 0, 0.05,
        kept2.ctypes.data_as(C.POINTER(C.c_uint64)), None, 0, native.HOST, offs.ctypes.data_as(C.c_void_p),
        cs.ctypes.data_as(C.c_void_p), modes.ctypes.data_as(C.c_void_p)))
    _same(codec.audit_last_encode(), want)            # before the fetch
    out = np.zeros(int(offs[2]), dtype=np.uint8)
    native._check(native.lib().cldn_hip_codec_fetch_output(codec._h, out.ctypes.data_as(C.c_void_p), out.size))
    assert out.tobytes() == np.concatenate(ref_streams).tobytes()    # the audit before it did not disturb the output
    _same(codec.audit_last_encode(), want)            # and after


def test_arguments(oracle):
    from cloudini_amd import native
    info, data = synth.lidar_xyzi(1000)
    codec = _codec(info)
    for lim in ([0.1, 0.1, -1.0, 0.0], [0.1, np.nan, 0.1, 0.0]):
        with pytest.raises(native.CloudiniHipError) as e:
            codec.audit_clouds_host([data], [data], limit=lim)
        assert e.value.code == -1
    with pytest.raises(native.CloudiniHipError) as e:
        codec.audit_streams_host([data], [data], stream_kind=2)
    assert e.value.code == -1
    _t, p, _c = _dev(data)
    read, pr = _dev_report(1, 4)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.audit_clouds_device(p, p, [1000], report_ptr=pr + 4)
    assert e.value.code == -1
    assert M.clean(info, codec.audit_clouds_host([data], [data]))
